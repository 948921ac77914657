"""Decoy windows for the tests that call a per-window entry point at a window index other than 0 (test infrastructure).

A handle concatenates the windows of a batch into global arrays; window w sits at the offsets kf_base / cam_base / lmk_base /
obs_base. An entry point that forgets one of them reads the rows of the window stored in front. A DECOY is a window put in front of
(or behind) the window under test whose rows differ from the target's at every index the target could alias, so that a forgotten
base reads wrong data, never equal data:
  - n_kf, n_lmk, obs_per_lmk, the trajectory length and the seed differ from every target's (so does the observation count);
  - it stores THREE cameras: an extra camera 0 (focal lengths x 1.05, its own T_s_f), then the rig's two, obs_cam shifted by one.
    Camera c of the target then aliases another camera, and cam_base is 3, not 2. cam_sigma differs on all three (the handle stores
    cameras with identical (K, T_s_f, sigma) once, and the oracle reads cam_sigma too). Every fifth left-camera observation is
    re-measured through camera 0, so that camera is in use and the decoy stays a consistent least-squares problem;
  - factor_type and has_imu are the target's: they are properties of the handle.
The targets are never modified: they are the windows the single-window tests already use, and their bars apply unchanged.

global_view() is the host emulation of a forgotten base that tests/test_window_index_cpu.py runs through the oracle: it proves that
each decoy used by tests/test_gpu_window_index.py moves the target's linearisation far beyond the 1e-10 parity bar."""
import numpy as np

import cov_helpers as ch
from frontend_helpers import landmark_optimization_window
from marg_helpers import with_lonely_landmarks
from sadvio_amd import capi, synthetic
from sadvio_amd.synthetic import T12_to_4, T_to_12, exp_so3
from vio_helpers import make_vio_window

PIXEL, ANGULAR = capi.FACTOR_PIXEL, capi.FACTOR_ANGULAR
SIGMA_SCALE = (3.0, 0.8, 1.3)        # pixel: the sigmas themselves; angular: factors on the rig's 1.5 / f


def add_decoy_camera(w, seed, variant=0):
    """w (from synthetic.make_window / make_vio_window) with an extra camera 0 in front of the rig's two. Two decoys of one batch
    take different variants: the extra camera's T_s_f and all three sigmas then differ between them as well."""
    rng = np.random.default_rng(seed + 5000)
    K0 = w.cam_K[0] * np.array([1.05, 1.05, 1.0, 1.0])
    D = np.eye(4)
    D[:3, :3] = exp_so3(np.array([0.01, -0.015, 0.008]))
    D[:3, 3] = np.array([0.03, -0.01, 0.005]) + 0.01 * variant
    T0 = D @ T12_to_4(w.cam_T_s_f[0])
    cam = (w.obs_cam + 1).astype(np.int32)
    meas = w.obs_meas.copy()
    sel = np.flatnonzero(cam == 1)[::5]
    assert len(sel) >= 3
    lmk_of = np.repeat(np.arange(w.n_lmk), np.diff(w.lmk_obs_ptr))
    for o in sel:
        pc = (T0 @ T12_to_4(w.truth["T_f_w"][w.obs_kf[o]]) @ np.append(w.truth["lmk"][lmk_of[o]], 1.0))[:3]
        uv = np.array([K0[0] * pc[0] / pc[2] + K0[2], K0[1] * pc[1] / pc[2] + K0[3]]) + rng.standard_normal(2)
        if w.factor_type == PIXEL:
            meas[o] = uv
        else:
            b = np.array([(uv[0] - K0[2]) / K0[0], (uv[1] - K0[3]) / K0[1], 1.0])
            meas[o] = b / np.linalg.norm(b)
        cam[o] = 0
    if w.factor_type == PIXEL:
        sigma = np.array(SIGMA_SCALE)
    else:
        f = 0.5 * (K0[:2].sum()), 0.5 * (w.cam_K[0, :2].sum()), 0.5 * (w.cam_K[1, :2].sum())
        sigma = np.array(SIGMA_SCALE) * 1.5 / np.array(f)
    w.cam_K = np.vstack([K0[None], w.cam_K])
    w.cam_T_s_f = np.vstack([T_to_12(T0)[None], w.cam_T_s_f])
    w.cam_sigma = sigma * (1.0 + 0.1 * variant)
    w.obs_cam, w.obs_meas = cam, meas
    w._keep = []
    return w


# (n_kf, n_lmk, obs_per_lmk, seed, length): no target of test_gpu_window_index.py has any of these n_kf / n_lmk / obs_per_lmk
_SHAPES = {"a": (7, 90, 3, 901, 7.0), "b": (9, 70, 7, 902, 13.0)}


def decoy(factor=PIXEL, which="a", vio=False):
    n_kf, n_lmk, opl, seed, length = _SHAPES[which]
    if vio:
        w = make_vio_window(n_kf=n_kf, n_lmk=n_lmk, obs_per_lmk=opl, seed=seed + 10, factor=factor, length=length)
    else:
        w = synthetic.make_window(n_kf=n_kf, n_lmk=n_lmk, obs_per_lmk=opl, seed=seed, factor=factor, length=length)
    return add_decoy_camera(w, seed, variant={"a": 0, "b": 1}[which])


# ---- the targets (the windows of the single-window tests, built as those tests build them) ----------------------------------------
def lin_target(factor, empty=None):
    """Window of the linearize parity test, smaller; empty = "first" / "last": that landmark keeps no observation."""
    w = synthetic.make_window(n_kf=5, n_lmk=150, seed=3, factor=factor)
    if empty is not None:
        l = 0 if empty == "first" else w.n_lmk - 1
        keep = np.ones(w.n_obs, dtype=bool)
        keep[w.lmk_obs_ptr[l]:w.lmk_obs_ptr[l + 1]] = False
        w = ch._keep_observations(w, keep)
    return w


def chi2_target(factor):
    """test_gpu_frontend.py::test_landmark_chi2_gate's window."""
    w = landmark_optimization_window(factor=factor, seed=57 + factor)
    if factor == ANGULAR:
        w.obs_meas /= np.linalg.norm(w.obs_meas, axis=1, keepdims=True)
    w.lmk_p = w.lmk_p.copy()
    w.lmk_p[3] += np.array([0.0, 0.0, -60.0])
    w.lmk_p[7] += np.array([40.0, 0.0, 0.0])
    return w


def rel_target(factor):
    """test_gpu_relative_batch.py::test_parity_all_ordered_pairs' window."""
    return synthetic.make_window(n_kf=5, n_lmk=300, obs_per_lmk=6, seed=14, factor=factor)


def rel_other(factor):
    """Another window of different size for the csr_win test. It follows the target in one batch, so it carries the three decoy
    cameras too (two windows of the plain rig side by side could swap their camera rows unnoticed); it is itself checked against
    the oracle."""
    return add_decoy_camera(synthetic.make_window(n_kf=4, n_lmk=120, obs_per_lmk=5, seed=15, factor=factor), 15, variant=2)


def marg_vo_target(factor):
    """test_gpu_marg.py::test_vo_window_oldest_keyframe's window and arguments."""
    w = synthetic.make_window(n_kf=6, n_lmk=400, seed=71, factor=factor)
    kf0 = w.n_kf - 1
    w = with_lonely_landmarks(w, kf0, 12)
    keep, marg = synthetic.pre_marginalize(w, kf0)
    return w, dict(kf_marg=kf0, lmk_marg=marg, lmk_keep=keep, priors=w.pose_priors)


def marg_vio_target():
    """test_gpu_marg.py::test_vio_window_with_imu_and_previous_prior's window and arguments."""
    w = make_vio_window(n_kf=6, n_lmk=400, seed=72)
    kf0, kf1 = w.n_kf - 1, w.n_kf - 2
    w = with_lonely_landmarks(w, kf0, 10)
    keep, marg = synthetic.pre_marginalize(w, kf0)
    imu = [f for f in w.imu_factors if f["kf_i"] == kf0 and f["kf_j"] == kf1][0]
    rng = np.random.default_rng(7)
    prev_l = np.array(keep[:6] + marg[:2], dtype=np.int32)
    nl = 15 + 3 * len(prev_l)
    last = {"J": rng.standard_normal((nl - 3, nl)), "r0": 0.3 * rng.standard_normal(nl - 3), "kf_keep": kf0, "kf_col": 0,
            "lmk_index": prev_l, "lmk_col": (15 + 3 * np.arange(len(prev_l))).astype(np.int32)}
    return w, dict(kf_marg=kf0, lmk_marg=marg, lmk_keep=keep, kf_keep=kf1, marg_has_imu=True, imu=imu, priors=w.pose_priors, last=last)


def prior_pipeline_target():
    """test_gpu_marg.py::test_device_prior_feeds_the_next_solve: (w, marginalize arguments, w2 without its dense prior)."""
    w = with_lonely_landmarks(make_vio_window(n_kf=6, n_lmk=400, seed=73), 5, 10)
    kf0, kf1 = w.n_kf - 1, w.n_kf - 2
    keep, marg = synthetic.pre_marginalize(w, kf0)
    imu = [f for f in w.imu_factors if f["kf_i"] == kf0 and f["kf_j"] == kf1][0]
    args = dict(kf_marg=kf0, lmk_marg=marg, lmk_keep=keep, kf_keep=kf1, marg_has_imu=True, imu=imu, priors=w.pose_priors)
    w2 = with_lonely_landmarks(make_vio_window(n_kf=6, n_lmk=400, seed=73), 5, 10)
    w2.pose_priors = []
    w2.kf_const = np.zeros(w2.n_kf, dtype=np.uint8); w2.kf_const[kf0] = 1
    w2.imu_factors = [f for f in w2.imu_factors if f["kf_i"] != kf0]
    return w, args, w2


# ---- every (windows in front, target) pair of test_gpu_window_index.py, for the CPU proof ------------------------------------------
def pairs_used():
    """[(name, [windows stored in front of the target], target)] — the GPU tests build their batches from the same functions."""
    out = []
    for f, fn in ((PIXEL, "pixel"), (ANGULAR, "angular")):
        a, b = decoy(f, "a"), decoy(f, "b")
        out += [(f"linearize {fn} [a | plain]", [a], lin_target(f)),
                (f"linearize {fn} [a, b | last landmark empty]", [a, b], lin_target(f, "last")),
                (f"linearize {fn} [b | first landmark empty]", [b], lin_target(f, "first")),
                (f"landmark_chi2 {fn} [a, b | target]", [a, b], chi2_target(f)),
                (f"relative {fn} [a, b | target]", [a, b], rel_target(f)),
                (f"relative {fn} csr [a | target]", [a], rel_target(f)),
                (f"relative {fn} csr [a, target | other]", [a, rel_target(f)], rel_other(f)),
                (f"relative {fn} csr second batch [b | other]", [b], rel_other(f)),
                (f"marginalize vo {fn} [a | target]", [a], marg_vo_target(f)[0])]
    va, vb = decoy(PIXEL, "a", vio=True), decoy(PIXEL, "b", vio=True)
    w, _, w2 = prior_pipeline_target()
    out += [("marginalize vio [vio a | target]", [va], marg_vio_target()[0]),
            ("dense prior batch 1 [vio a | w]", [va], w),
            ("dense prior batch 2 [vio b | w2]", [vb], w2)]
    a = decoy(PIXEL, "a")
    out += [("covariance [a | pixel_vo]", [a], ch.window_pixel_vo()),
            ("covariance [a, pixel_vo | lmk600]", [a, ch.window_pixel_vo()], ch.window_lmk600()),
            ("covariance [a, pixel_vo, lmk600 | obs64]", [a, ch.window_pixel_vo(), ch.window_lmk600()], ch.window_obs64()),
            ("covariance [angular a | angular_vo]", [decoy(ANGULAR, "a")], ch.window_angular_vo())]
    _, _, w2c, _ = ch.vio_marg_step()
    out.append(("covariance [vio a | vio window]", [va], w2c))
    return out


def global_view(front, target, drop=None, wrong=0):
    """The target as the handle stores it: key-frames and cameras of [front..., target] concatenated, the target's landmarks and
    observations indexing them through its bases. drop = "kf" / "cam" / "lmk" / "obs": that base is replaced by the base of window
    `wrong` of the batch (0: the base is forgotten altogether) — the host emulation of the fault a decoy exists to expose.
    oracle.linearize of the view with drop = None equals that of the target alone."""
    ws = list(front) + [target]
    kf_b = np.concatenate([[0], np.cumsum([x.n_kf for x in ws])]).astype(int)
    cam_b = np.concatenate([[0], np.cumsum([x.n_cam for x in ws])]).astype(int)
    lmk_b = np.concatenate([[0], np.cumsum([x.n_lmk for x in ws])]).astype(int)
    obs_b = np.concatenate([[0], np.cumsum([x.n_obs for x in ws])]).astype(int)
    t = len(ws) - 1
    base = {"kf": kf_b[t], "cam": cam_b[t], "lmk": lmk_b[t], "obs": obs_b[t]}
    if drop is not None:
        base[drop] = {"kf": kf_b, "cam": cam_b, "lmk": lmk_b, "obs": obs_b}[drop][wrong]
    g_kf = np.concatenate([kf_b[i] + x.obs_kf for i, x in enumerate(ws)]).astype(np.int32)
    g_cam = np.concatenate([cam_b[i] + x.obs_cam for i, x in enumerate(ws)]).astype(np.int32)
    g_meas = np.concatenate([x.obs_meas for x in ws])
    g_lmk = np.concatenate([x.lmk_p for x in ws])
    n_o, n_l = target.n_obs, target.n_lmk
    rows = slice(base["obs"], base["obs"] + n_o)
    okf, ocam = g_kf[rows] - kf_b[t] + base["kf"], g_cam[rows] - cam_b[t] + base["cam"]
    if drop == "obs":      # the rows of another window carry that window's bases
        okf, ocam = g_kf[rows], g_cam[rows]
    return capi.FlatWindow(
        kf_T_f_w=np.concatenate([x.kf_T_f_w for x in ws]), kf_const=np.concatenate([x.kf_const for x in ws]),
        cam_K=np.concatenate([x.cam_K for x in ws]), cam_T_s_f=np.concatenate([x.cam_T_s_f for x in ws]),
        cam_sigma=np.concatenate([x.cam_sigma for x in ws]), lmk_p=g_lmk[base["lmk"]:base["lmk"] + n_l].copy(),
        lmk_obs_ptr=target.lmk_obs_ptr, obs_kf=okf.astype(np.int32), obs_cam=ocam.astype(np.int32), obs_meas=g_meas[rows].copy(),
        factor_type=target.factor_type, has_imu=0)
