"""Windows of non-pinhole rigs for the tests of sadvio_ba_landmark_chi2_models (test infrastructure).

model_window() builds the smallest window at which the gate can still go wrong: 3 key-frames, 2 cameras of DIFFERENT kinds, 65
landmarks (the 64-lane workgroup boundary is crossed) with tracks of 1, 2 and 5 observations, some of them not in key-frame
order (the handle then stores them permuted, so obs_uv and obs_chi2 go through its permutation). The four RIGS together hold
every kind, alpha 0.3 and 0.7 for omni and double sphere, and omni with and without distortion. Landmarks with a fixed role:
  BEHIND      z = -2 in the camera frame: fails on every model
  SHALLOW     z = 0.05: passes the fisheye laws' depth test (0.01), fails the 0.1 of the others
  TOO_SHALLOW z = 0.005: fails on every model
  OUTSIDE     moved 40 m sideways: valid arithmetic, pixel outside the image
  NEAR_AXIS   one observation at theta = 1e-3 off the axis (acos amplifies by 1 / theta there; its own bar on the CPU)
Every other landmark is drawn so that each of its observations is valid, inside the image and, on a fisheye camera, at least
MIN_THETA off the axis. The omni / double-sphere cone test z <= -w d cannot fail behind their early z < 0.1 return for
0 < alpha < 1; alpha 0.3 and 0.7 run both branches of w.

decoys() gives the two windows that sit in front of the target in the window-index test: other key-frame, landmark and CAMERA
counts (3 and 1) and other kinds at every index the target's cameras could alias (the pattern of tests/batch_helpers.py)."""
import numpy as np

import camera_models as cm
from sadvio_amd import capi
from sadvio_amd.synthetic import T12_to_4, T_to_12, exp_so3, inv4

PIXEL, ANGULAR = capi.FACTOR_PIXEL, capi.FACTOR_ANGULAR
WIDTH, HEIGHT = 752.0, 480.0
MIN_THETA = 0.05
BEHIND, SHALLOW, OUTSIDE, NEAR_AXIS, TOO_SHALLOW = 4, 7, 11, 12, 16
N_LMK = 65
_D = (-0.05, 0.01, 0.001, -0.0005)


def _cam(kind, K, **kw):
    m = {"kind": kind, "width": WIDTH, "height": HEIGHT, "rmax": 1.0, "xi": 0.0, "alpha": 0.0, "distortion": 0, "D": (0.0, 0.0, 0.0, 0.0)}
    m.update(kw)
    return np.array(K, dtype=np.float64), m


CAMS = {
    "pinhole": _cam(cm.PINHOLE, (458.654, 457.296, 367.215, 248.375)),
    "equidistant": _cam(cm.EQUIDISTANT, (1.1, 1.1, 376.0, 240.0), rmax=300.0),
    "equisolid": _cam(cm.EQUISOLID, (1.05, 1.05, 370.5, 236.0), rmax=310.0),
    "stereographic": _cam(cm.STEREOGRAPHIC, (0.95, 0.95, 380.25, 244.5), rmax=290.0),
    "omni_a3": _cam(cm.OMNI, (300.0, 301.0, 376.0, 240.0), alpha=0.3, xi=0.3 / 0.7),
    "omni_a7_D": _cam(cm.OMNI, (305.0, 304.0, 372.0, 238.0), alpha=0.7, xi=0.7 / 0.3, distortion=1, D=_D),
    "ds_a3": _cam(cm.DOUBLE_SPHERE, (350.0, 352.0, 376.0, 240.0), alpha=0.3, xi=-0.2),
    "ds_a7": _cam(cm.DOUBLE_SPHERE, (348.0, 351.0, 371.0, 243.0), alpha=0.7, xi=0.1),
}
RIGS = {"pinhole_equidistant": ("pinhole", "equidistant"), "equisolid_stereographic": ("equisolid", "stereographic"),
        "omni": ("omni_a3", "omni_a7_D"), "double_sphere": ("ds_a3", "ds_a7")}


def _world_from_cam(T_f_w, T_s_f, pc):
    return (inv4(T12_to_4(T_f_w)) @ inv4(T12_to_4(T_s_f)) @ np.append(pc, 1.0))[:3]


def _theta(pc):
    return float(np.arccos(pc[2] / np.linalg.norm(pc)))


def model_window(cams, factor, seed=0, n_kf=3, n_lmk=N_LMK, roles=True, kf_free=True):
    """(window, models, obs_uv): cams = names of CAMS, one per camera of the rig. window.truth["role_obs"] lists the observations
    of the landmarks with a fixed role, window.truth["near_axis_obs"] the single near-axis one (or None)."""
    rng = np.random.default_rng(4100 + 17 * seed + 3 * n_kf + len(cams))
    n_cam = len(cams)
    K = np.array([CAMS[c][0] for c in cams])
    models = [dict(CAMS[c][1]) for c in cams]
    kf_T = []
    for k in range(n_kf):
        R = exp_so3(0.01 * rng.standard_normal(3))
        c = np.array([0.25 * k, 0.02 * k, 0.01 * k])
        T = np.eye(4); T[:3, :3] = R; T[:3, 3] = -R @ c
        kf_T.append(T_to_12(T))
    kf_T = np.array(kf_T)
    cam_T = []
    for c in range(n_cam):
        T = np.eye(4); T[:3, :3] = exp_so3(0.004 * rng.standard_normal(3)); T[:3, 3] = np.array([-0.11 * c, 0.002 * c, 0.001 * c])
        cam_T.append(T_to_12(T))
    cam_T = np.array(cam_T)
    combos_all = [(k, c) for k in range(n_kf) for c in range(n_cam)]

    def cam_point(p, k, c):
        return (T12_to_4(cam_T[c]) @ T12_to_4(kf_T[k]) @ np.append(p, 1.0))[:3]

    def good(p):
        for k, c in combos_all:
            pc = cam_point(p, k, c)
            u, v, ok = cm.project_camera(models[c], K[c], pc)
            if not ok or not (30.0 < u < WIDTH - 30.0 and 30.0 < v < HEIGHT - 30.0):
                return False
            if models[c]["kind"] in cm.FISHEYE and _theta(pc) < MIN_THETA + 0.015:
                return False
        return True

    fish = [c for c in range(n_cam) if models[c]["kind"] in cm.FISHEYE]
    special = {}
    if roles:
        special = {BEHIND: ([(2, 0), (2, n_cam - 1)], np.array([0.3, 0.2, -2.0])),
                   SHALLOW: ([(1, 0), (1, n_cam - 1)], np.array([0.02, 0.01, 0.05])),
                   TOO_SHALLOW: ([(0, 0), (0, n_cam - 1)], np.array([0.002, 0.001, 0.005])),
                   NEAR_AXIS: ([(1, fish[-1] if fish else 0)], np.array([0.004, 0.003, 5.0]))}
    truth, est, ptr, obs_kf, obs_cam, uv, role_obs, near = [], [], [0], [], [], [], [], None
    for l in range(n_lmk):
        while True:
            p = np.array([rng.uniform(-1.2, 1.6), rng.uniform(-0.9, 0.9), rng.uniform(3.0, 6.0)])
            if good(p):
                break
        n = (1, 2, 5)[l % 3] if len(combos_all) >= 5 else min((1, 2, 5)[l % 3], len(combos_all))
        start = l % len(combos_all)
        combos = [combos_all[(start + i) % len(combos_all)] for i in range(n)]     # wraps: not in key-frame order for some
        pe = p + 0.01 * rng.standard_normal(3)
        noise = 0.7
        if l in special:
            combos, pc = special[l]
            pe = _world_from_cam(kf_T[combos[0][0]], cam_T[combos[0][1]], pc)
            if l == NEAR_AXIS:
                p, noise = pe.copy(), 0.2
        elif roles and l == OUTSIDE:
            pe = p + np.array([40.0, 0.0, 0.0])
        for k, c in combos:
            u, v, ok = cm.project_camera(models[c], K[c], cam_point(p, k, c))
            assert ok
            if roles and (l in special or l == OUTSIDE):
                role_obs.append(len(obs_kf))
                if l == NEAR_AXIS:
                    near = len(obs_kf)
            obs_kf.append(k); obs_cam.append(c)
            uv.append(np.array([u, v]) + noise * rng.standard_normal(2))
        truth.append(p); est.append(pe); ptr.append(len(obs_kf))
    uv = np.array(uv)
    obs_cam = np.array(obs_cam, dtype=np.int32)
    if factor == PIXEL:
        meas, sigma = uv.copy(), np.array([1.0, 1.3, 0.8][:n_cam])
    else:   # the bearing the host layer stores: getRayCamera of the feature's pixel through its own model
        meas = np.array([cm.ray_camera(models[c], K[c], q[0], q[1]) for c, q in zip(obs_cam, uv)], dtype=np.float64)
        f = np.array([K[c, 0] * models[c]["rmax"] if models[c]["kind"] in cm.FISHEYE else 0.5 * (K[c, 0] + K[c, 1]) for c in range(n_cam)])
        sigma = 1.5 / f
    kf_const = np.zeros(n_kf, dtype=np.uint8)
    kf_const[-1] = 1
    if not kf_free:
        kf_const[:] = 1
    w = capi.FlatWindow(kf_T_f_w=kf_T, kf_const=kf_const, cam_K=K, cam_T_s_f=cam_T, cam_sigma=sigma, lmk_p=np.array(est),
                        lmk_obs_ptr=np.array(ptr, dtype=np.int32), obs_kf=np.array(obs_kf, dtype=np.int32), obs_cam=obs_cam,
                        obs_meas=meas, factor_type=factor, has_imu=0)
    w.truth = {"lmk": np.array(truth), "role_obs": role_obs, "near_axis_obs": near}
    return w, models, uv


def rig_window(rig, factor):
    """The window of one of the four RIGS. Pixel windows hold their key-frames constant: the pixel factor projects with K only,
    and a pose solve against fisheye pixels would say nothing about the gate."""
    return model_window(RIGS[rig], factor, seed=list(RIGS).index(rig), kf_free=factor == ANGULAR)


def fixed_deltas(w, seed=1):
    """Deltas of the size a solve produces, fixed, so that the CPU checks see exactly what the GPU test evaluates."""
    rng = np.random.default_rng(900 + seed)
    return 0.004 * rng.standard_normal((w.n_kf, 6)), 0.01 * rng.standard_normal((w.n_lmk, 3))


def decoys(factor):
    """Two windows stored in front of the target: 3 cameras (double sphere, omni, stereographic) and 1 camera (equisolid)."""
    a = model_window(("ds_a7", "omni_a3", "stereographic"), factor, seed=21, n_kf=4, n_lmk=40, roles=False, kf_free=factor == ANGULAR)
    b = model_window(("equisolid",), factor, seed=22, n_kf=5, n_lmk=30, roles=False, kf_free=factor == ANGULAR)
    return a, b


def target(factor):
    return rig_window("pinhole_equidistant", factor)


def pinhole_models(w, wh=None):
    return [{"kind": cm.PINHOLE, "width": (2.0 * w.cam_K[c, 2] if wh is None else wh[c][0]), "height": (2.0 * w.cam_K[c, 3] if wh is None else wh[c][1])}
            for c in range(w.n_cam)]
