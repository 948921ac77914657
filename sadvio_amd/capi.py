"""ctypes binding of the C ABI declared in include/sadvio_ba.h.

This module is harness plumbing (tests, bench, smoke): the product is `libsadvio_ba.so`, whose
entry points are what a SaDVIO `isae::AOptimizer` adapter binds. There is no CPU
fallback: loading fails loudly when the HIP library has not been built, and every compute call
returns SADVIO_E_NO_DEVICE / SADVIO_E_HIP when no gfx950 device is usable.
"""
from __future__ import annotations

import ctypes as C
import os
from dataclasses import dataclass, field
from typing import List, Optional, Sequence

import numpy as np

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.environ.get("SADVIO_BA_LIB") or os.path.join(_HERE, "csrc", "libsadvio_ba.so")   # override: A/B measurement builds

SADVIO_OK = 0
CFG_LONG_TRACKS = 1   # sadvio_ba_config.reserved: SADVIO_CFG_LONG_TRACKS
CFG_LONG_TRACK_PRIORS = 2   # ... SADVIO_CFG_LONG_TRACK_PRIORS (with CFG_LONG_TRACKS)
CFG_LONG_TRACK_COVARIANCE = 4   # ... SADVIO_CFG_LONG_TRACK_COVARIANCE (with CFG_LONG_TRACKS)
CFG_LONG_TRACK_BATCH = 8   # ... SADVIO_CFG_LONG_TRACK_BATCH (with CFG_LONG_TRACKS)
E_INVALID_ARG, E_NOT_USABLE, E_HIP, E_RCCL, E_NO_DEVICE, E_STATE, E_REFUSED = -1, -2, -3, -4, -5, -6, -7
FACTOR_PIXEL, FACTOR_ANGULAR = 0, 1
TERM_NAMES = {0: "NO_CONVERGENCE", 1: "FUNCTION_TOL", 2: "PARAMETER_TOL", 3: "GRADIENT_TOL", 4: "MIN_RADIUS",
              5: "FAILURE"}

_dp = C.POINTER(C.c_double)
_ip = C.POINTER(C.c_int32)
_lp = C.POINTER(C.c_int64)
_bp = C.POINTER(C.c_uint8)


class Config(C.Structure):
    _fields_ = [("device", C.c_int32), ("profile_kernels", C.c_int32), ("use_graph", C.c_int32),
                ("reserved", C.c_int32)]


# int fn(void* ctx, double* device_buf, int64 count, void* hip_stream): in-place sum all-reduce, enqueued on the stream
ALLREDUCE_FN = C.CFUNCTYPE(C.c_int, C.c_void_p, C.c_void_p, C.c_int64, C.c_void_p)
RCCL_ID_BYTES = 128


class FlatWindowC(C.Structure):
    _fields_ = [
        ("n_kf", C.c_int32), ("n_cam", C.c_int32), ("n_lmk", C.c_int32), ("n_obs", C.c_int32),
        ("factor_type", C.c_int32), ("has_imu", C.c_int32),
        ("kf_id", _lp), ("kf_T_f_w", _dp), ("kf_const", _bp), ("kf_vel", _dp), ("kf_ba", _dp), ("kf_bg", _dp),
        ("cam_K", _dp), ("cam_T_s_f", _dp), ("cam_sigma", _dp),
        ("lmk_id", _lp), ("lmk_p", _dp), ("lmk_const", _bp), ("lmk_obs_ptr", _ip),
        ("obs_kf", _ip), ("obs_cam", _ip), ("obs_meas", _dp),
    ]


class ImuFactorC(C.Structure):
    _fields_ = [
        ("kf_i", C.c_int32), ("kf_j", C.c_int32), ("dt", C.c_double),
        ("delta_R", C.c_double * 9), ("delta_v", C.c_double * 3), ("delta_p", C.c_double * 3),
        ("J_dR_bg", C.c_double * 9), ("J_dv_ba", C.c_double * 9), ("J_dv_bg", C.c_double * 9),
        ("J_dp_ba", C.c_double * 9), ("J_dp_bg", C.c_double * 9), ("cov", C.c_double * 81),
        ("bacc_noise", C.c_double), ("bgyr_noise", C.c_double),
    ]


class ViInitProblemC(C.Structure):
    _fields_ = [("n_frames", C.c_int32), ("n_factors", C.c_int32), ("T_f_w", C.POINTER(C.c_double)),
                ("vel", C.POINTER(C.c_double)), ("factors", C.POINTER(ImuFactorC)), ("optim_scale", C.c_int32),
                ("optim_bias", C.c_int32), ("sigma_dba", C.c_double), ("sigma_dbg", C.c_double)]


class ViInitResultC(C.Structure):
    _fields_ = [("r_wi", C.c_double * 2), ("lambda_", C.c_double), ("dba", C.c_double * 3), ("dbg", C.c_double * 3),
                ("R_w_i", C.c_double * 9), ("scale", C.c_double)]


class NoFovProblemC(C.Structure):
    _fields_ = [("n_lmk", C.c_int32), ("n_obs", C.c_int32), ("n_frames", C.c_int32), ("n_cam", C.c_int32), ("cam0", C.c_int32),
                ("fix_scale", C.c_int32), ("frame_T_f_w", _dp), ("cam_T_s_f", _dp), ("T_cam0_cam0p", _dp), ("info_scale", C.c_double),
                ("gate", C.c_double), ("lmk_p", _dp), ("scale_bearing", _dp), ("scale_cam", _ip), ("lmk_obs_ptr", _ip),
                ("obs_frame", _ip), ("obs_cam", _ip), ("obs_bearing", _dp)]


class NoFovResultC(C.Structure):
    _fields_ = [("lambda_", C.c_double), ("usable", C.c_int32), ("scale_fixed", C.c_int32), ("n_inliers", C.c_int32),
                ("pad", C.c_int32)]


class LineSetC(C.Structure):
    _fields_ = [("n_line", C.c_int32), ("n_obs", C.c_int32), ("line_id", _lp), ("line_T_w_l", _dp), ("line_model", _dp),
                ("line_const", _bp), ("line_obs_ptr", _ip), ("obs_kf", _ip), ("obs_cam", _ip), ("obs_meas", _dp)]


class PosePriorC(C.Structure):
    _fields_ = [("kf", C.c_int32), ("pad", C.c_int32), ("T_prior", C.c_double * 12), ("inf_diag", C.c_double * 6)]


class SparsePriorC(C.Structure):
    _fields_ = [("type", C.c_int32), ("kf", C.c_int32), ("lmk0", C.c_int32), ("lmk1", C.c_int32),
                ("T_prior", C.c_double * 12), ("v_prior", C.c_double * 3), ("ba_prior", C.c_double * 3),
                ("bg_prior", C.c_double * 3), ("delta", C.c_double * 3), ("sqrt_inf", C.c_double * 225),
                ("kf_b", C.c_int32), ("pad", C.c_int32)]


SPARSE_IMU_PRIOR, SPARSE_POSE_TO_LMK, SPARSE_LMK_PRIOR, SPARSE_LMK_TO_LMK, SPARSE_RELATIVE_POSE = 0, 1, 2, 3, 4


class MargRequestC(C.Structure):
    _fields_ = [("kf_marg", C.c_int32), ("kf_keep", C.c_int32), ("marg_has_imu", C.c_int32), ("n_marg", C.c_int32),
                ("lmk_marg", _ip), ("n_keep", C.c_int32), ("lmk_keep", _ip), ("imu", C.POINTER(ImuFactorC)),
                ("n_prior", C.c_int32), ("priors", C.POINTER(PosePriorC)), ("last_n_full", C.c_int32), ("last_n", C.c_int32),
                ("last_J", _dp), ("last_r0", _dp), ("last_kf", C.c_int32), ("last_kf_col", C.c_int32),
                ("last_n_keep", C.c_int32), ("last_lmk_index", _ip), ("last_lmk_col", _ip),
                ("eig_cut_mode", C.c_int32), ("prior_form", C.c_int32)]


class PriorInfoC(C.Structure):
    _fields_ = [("valid", C.c_int32), ("n_full", C.c_int32), ("n", C.c_int32), ("form", C.c_int32)]


class CovRequestC(C.Structure):
    _fields_ = [("n_kf", C.c_int32), ("kf", _ip), ("n_pair", C.c_int32), ("pair_a", _ip), ("pair_b", _ip), ("n_lmk", C.c_int32),
                ("lmk", _ip)]


class CovBatchItemC(C.Structure):
    _fields_ = [("w", C.c_int32), ("status", C.c_int32), ("n_lmk_singular", C.c_int32), ("route", C.c_int32), ("rq", CovRequestC),
                ("kf_cov", _dp), ("pair_cov", _dp), ("lmk_cov", _dp)]


class CovCrossRequestC(C.Structure):
    _fields_ = [("n", C.c_int32), ("kf", _ip), ("lmk", _ip), ("cam", _ip), ("meas", _dp)]


COV_ROUTE_NONE, COV_ROUTE_LDS, COV_ROUTE_DENSE, COV_ROUTE_BAND, COV_ROUTE_BORDER = 0, 1, 2, 3, 4   # SADVIO_COV_ROUTE_*
CROSS_OK, CROSS_LMK_SINGULAR, CROSS_PROJ_INVALID = 0, 1, 2                    # SADVIO_CROSS_*
PRIOR_RESIDENT = -1
# SADVIO_EIG_CUT_*: the C ABI's default (a zero-initialised request) is the reference's absolute 1e-12; this harness and the
# oracle's wrapper default to "noise_floor" because the parity tests compare n_full, which only that mode makes reproducible
# across eigen-solvers (sadvio_ba.h); tests of the reference mode pass eig_cut="reference" on both sides.
EIG_CUT = {"reference": 0, "noise_floor": 1}
PRIOR_FORM = {"eigen": 0, "cholesky": 1}          # SADVIO_PRIOR_FORM_*


class CameraModelC(C.Structure):
    """sadvio_camera_model: one camera of sadvio_ba_landmark_chi2_models (fx fy cx cy come from the window's cam_K)."""
    _fields_ = [("kind", C.c_int32), ("distortion", C.c_int32), ("width", C.c_double), ("height", C.c_double),
                ("rmax", C.c_double), ("xi", C.c_double), ("alpha", C.c_double), ("D", C.c_double * 4)]


CAM_PINHOLE, CAM_FISHEYE_EQUIDISTANT, CAM_FISHEYE_EQUISOLID, CAM_FISHEYE_STEREOGRAPHIC, CAM_OMNI, CAM_DOUBLE_SPHERE = range(6)


def camera_models_c(models):
    """A (CameraModelC * n) array from CameraModelC instances or dicts with its fields (absent fields: 0, rmax 1)."""
    arr = (CameraModelC * max(1, len(models)))()
    for i, m in enumerate(models):
        if isinstance(m, CameraModelC):
            C.memmove(C.byref(arr[i]), C.byref(m), C.sizeof(CameraModelC))
            continue
        a = arr[i]
        a.kind, a.distortion = int(m["kind"]), int(m.get("distortion", 0))
        a.width, a.height, a.rmax = float(m["width"]), float(m["height"]), float(m.get("rmax", 1.0))
        a.xi, a.alpha = float(m.get("xi", 0.0)), float(m.get("alpha", 0.0))
        a.D[:] = [float(x) for x in m.get("D", (0.0, 0.0, 0.0, 0.0))]
    return arr


class MargResultC(C.Structure):
    _fields_ = [("m", C.c_int32), ("n", C.c_int32), ("n_full", C.c_int32), ("kf_col", C.c_int32),
                ("sweeps_mm", C.c_int32), ("sweeps_k", C.c_int32)]


class SolveOptions(C.Structure):
    _fields_ = [
        ("max_num_iterations", C.c_int32), ("jacobi_scaling", C.c_int32),
        ("max_num_consecutive_invalid_steps", C.c_int32), ("reserved", C.c_int32),
        ("function_tolerance", C.c_double), ("gradient_tolerance", C.c_double),
        ("parameter_tolerance", C.c_double), ("initial_trust_region_radius", C.c_double),
        ("max_trust_region_radius", C.c_double), ("min_trust_region_radius", C.c_double),
        ("min_lm_diagonal", C.c_double), ("max_lm_diagonal", C.c_double), ("min_relative_decrease", C.c_double),
        ("huber_a", C.c_double), ("max_solver_time_in_seconds", C.c_double),
    ]


class SolveSummary(C.Structure):
    _fields_ = [
        ("iterations", C.c_int32), ("num_successful_steps", C.c_int32), ("num_unsuccessful_steps", C.c_int32),
        ("termination", C.c_int32), ("initial_cost", C.c_double), ("final_cost", C.c_double),
        ("fixed_cost", C.c_double), ("final_radius", C.c_double),
    ]

    def as_dict(self):
        return {k: getattr(self, k) for k, _ in self._fields_}


def reference_options() -> SolveOptions:
    """The reference's hard-coded options (AOptimizer.cpp:315-323) + Ceres 2.2.0 defaults."""
    o = SolveOptions()
    o.max_num_iterations = 20
    o.jacobi_scaling = 1
    o.max_num_consecutive_invalid_steps = 5
    o.function_tolerance = 1e-3
    o.gradient_tolerance = 1e-10
    o.parameter_tolerance = 1e-8
    o.initial_trust_region_radius = 1e4
    o.max_trust_region_radius = 1e16
    o.min_trust_region_radius = 1e-32
    o.min_lm_diagonal = 1e-6
    o.max_lm_diagonal = 1e32
    o.min_relative_decrease = 1e-3
    return o


def landmark_optimization_options() -> SolveOptions:
    """AOptimizer::landmarkOptimization (AOptimizer.cpp:98-119): Huber(sqrt(1.345)), 10 iterations; the caller marks
    every key-frame constant."""
    o = reference_options()
    o.max_num_iterations = 10
    o.huber_a = 1.345 ** 0.5
    return o


def single_frame_options(vi: bool = False) -> SolveOptions:
    """singleFrameOptimization (AOptimizer.cpp:152-174: no loss, 5 iterations) / singleFrameVIOptimization
    (:219-257: Huber on the visual factors, 5 iterations, 5 ms solver-time cap)."""
    o = reference_options()
    o.max_num_iterations = 5
    o.huber_a = 1.345 ** 0.5 if vi else 0.0
    o.max_solver_time_in_seconds = 0.005 if vi else 0.0
    return o


def viinit_options() -> SolveOptions:
    """AOptimizer::VIInit (AOptimizer.cpp:518-528): LM, 50 iterations, function_tolerance 1e-3, no loss."""
    o = reference_options()
    o.max_num_iterations = 50
    return o


def make_viinit_problem(T_f_w, vel, factors, optim_scale=False, optim_bias=False, sigma_dba=1.0, sigma_dbg=1.0):
    """(ViInitProblemC, keep-alive tuple) from arrays + a list of IMU factor dicts (kf_i / kf_j index the frames)."""
    T = np.ascontiguousarray(T_f_w, dtype=np.float64).reshape(-1, 12)
    v = np.ascontiguousarray(vel, dtype=np.float64).reshape(-1, 3)
    assert T.shape[0] == v.shape[0]
    arr = (ImuFactorC * max(1, len(factors)))()
    for i, f in enumerate(factors):
        fill_imu_factor(arr[i], f)
    P = ViInitProblemC(T.shape[0], len(factors), T.ctypes.data_as(_dp), v.ctypes.data_as(_dp), arr, int(optim_scale),
                       int(optim_bias), float(sigma_dba), float(sigma_dbg))
    return P, (T, v, arr)


def viinit_result_to_dict(rc, s, r: ViInitResultC, dv) -> dict:
    return {"rc": rc, "summary": s, "r_wi": np.array(r.r_wi[:]), "lambda": float(r.lambda_), "dba": np.array(r.dba[:]),
            "dbg": np.array(r.dbg[:]), "R_w_i": np.array(r.R_w_i[:]).reshape(3, 3), "scale": float(r.scale), "dv": dv}


def nofov_options() -> SolveOptions:
    """landmarkOptimizationNoFov (AngularAdjustmentCERESAnalytic.cpp:753, :857-868): LM, 20 iterations, function_tolerance
    1e-3, HuberLoss(sqrt(1.345)) on the visual factors (never on the scale prior)."""
    o = reference_options()
    o.huber_a = 1.345 ** 0.5
    return o


def make_nofov_problem(frame_T_f_w, cam_T_s_f, T_cam0_cam0p, lmk_p, scale_bearing, scale_cam, lmk_obs_ptr, obs_frame, obs_cam,
                       obs_bearing, cam0=0, fix_scale=-1, info_scale=0.0, gate=0.02):
    """(NoFovProblemC, keep-alive tuple) from arrays; see sadvio_nofov_problem in include/sadvio_ba.h."""
    d = lambda a, m: np.ascontiguousarray(a, dtype=np.float64).reshape(-1, m)
    i = lambda a: np.ascontiguousarray(a, dtype=np.int32).reshape(-1)
    T = d(frame_T_f_w, 12); Ts = d(cam_T_s_f, 12); Tm = d(T_cam0_cam0p, 12)
    lp = d(lmk_p, 3); sb = d(scale_bearing, 3); sc = i(scale_cam); ptr = i(lmk_obs_ptr); of = i(obs_frame); oc = i(obs_cam)
    ob = d(obs_bearing, 3)
    ip = lambda a: a.ctypes.data_as(_ip)
    P = NoFovProblemC(lp.shape[0], of.shape[0], T.shape[0], Ts.shape[0], int(cam0), int(fix_scale), _ptr(T), _ptr(Ts), _ptr(Tm),
                      float(info_scale), float(gate), _ptr(lp), _ptr(sb), ip(sc), ip(ptr), ip(of), ip(oc), _ptr(ob))
    return P, (T, Ts, Tm, lp, sb, sc, ptr, of, oc, ob)


def gn_options(iters: int = 10) -> SolveOptions:
    """BASELINE.json config 2 wording, "GN 10 iters": a fixed number of step attempts with every
    early-exit test disabled (trust-region schedule unchanged; at radius 1e4 the damping is ~1e-4
    relative, i.e. Gauss-Newton steps)."""
    o = reference_options()
    o.max_num_iterations = iters
    o.function_tolerance = 0.0
    o.gradient_tolerance = 0.0
    o.parameter_tolerance = 0.0
    return o


def _c(a: Optional[np.ndarray], dtype, ptr):
    if a is None:
        return None, ptr()
    arr = np.ascontiguousarray(a, dtype=dtype)
    return arr, arr.ctypes.data_as(ptr)


@dataclass
class FlatWindow:
    """Numpy-side holder of one flattened window (see sadvio_flat_window in include/sadvio_ba.h)."""
    kf_T_f_w: np.ndarray           # [n_kf,12]
    kf_const: np.ndarray           # [n_kf] uint8
    cam_K: np.ndarray              # [n_cam,4]
    cam_T_s_f: np.ndarray          # [n_cam,12]
    cam_sigma: np.ndarray          # [n_cam]
    lmk_p: np.ndarray              # [n_lmk,3]
    lmk_obs_ptr: np.ndarray        # [n_lmk+1] int32
    obs_kf: np.ndarray             # [n_obs] int32
    obs_cam: np.ndarray            # [n_obs] int32
    obs_meas: np.ndarray           # [n_obs,2|3]
    factor_type: int = FACTOR_PIXEL
    has_imu: int = 0
    kf_id: Optional[np.ndarray] = None
    lmk_id: Optional[np.ndarray] = None
    lmk_const: Optional[np.ndarray] = None
    kf_vel: Optional[np.ndarray] = None
    kf_ba: Optional[np.ndarray] = None
    kf_bg: Optional[np.ndarray] = None
    pose_priors: List[tuple] = field(default_factory=list)   # (kf, T_prior[12], inf_diag[6])
    imu_factors: List[dict] = field(default_factory=list)    # dicts with the ImuFactorC fields
    sparse_priors: List[dict] = field(default_factory=list)  # dicts with the SparsePriorC fields (NFR factors)
    lines: Optional[dict] = None         # linexd landmarks: T_w_l [n,12], model [n,6], obs_ptr, obs_kf, obs_cam, obs_meas [n_obs,4|6] (+ id, const)
    dense_prior: Optional[dict] = None   # MarginalizationFactor: J [n_full,n], r0, kf_keep, kf_col, lmk_index, lmk_col
    truth: dict = field(default_factory=dict)                # generator ground truth (not uploaded)
    _keep: list = field(default_factory=list, repr=False)

    @property
    def n_kf(self): return int(self.kf_T_f_w.shape[0])
    @property
    def n_cam(self): return int(self.cam_K.shape[0])
    @property
    def n_lmk(self): return int(self.lmk_p.shape[0])
    @property
    def n_obs(self): return int(self.obs_kf.shape[0])

    def to_c(self) -> FlatWindowC:
        if self.kf_id is None:
            self.kf_id = np.arange(self.n_kf, dtype=np.int64)
        if self.lmk_id is None:
            self.lmk_id = np.arange(self.n_lmk, dtype=np.int64)
        w = FlatWindowC()
        w.n_kf, w.n_cam, w.n_lmk, w.n_obs = self.n_kf, self.n_cam, self.n_lmk, self.n_obs
        w.factor_type, w.has_imu = int(self.factor_type), int(self.has_imu)
        keep = []
        for name, dt, ptr in [("kf_id", np.int64, _lp), ("kf_T_f_w", np.float64, _dp), ("kf_const", np.uint8, _bp),
                              ("kf_vel", np.float64, _dp), ("kf_ba", np.float64, _dp), ("kf_bg", np.float64, _dp),
                              ("cam_K", np.float64, _dp), ("cam_T_s_f", np.float64, _dp),
                              ("cam_sigma", np.float64, _dp), ("lmk_id", np.int64, _lp), ("lmk_p", np.float64, _dp),
                              ("lmk_const", np.uint8, _bp), ("lmk_obs_ptr", np.int32, _ip),
                              ("obs_kf", np.int32, _ip), ("obs_cam", np.int32, _ip), ("obs_meas", np.float64, _dp)]:
            arr, p = _c(getattr(self, name), dt, ptr)
            keep.append(arr)
            setattr(w, name, p)
        self._keep = keep  # keep the contiguous copies alive as long as this object lives
        return w

    def sparse_c(self):
        arr = (SparsePriorC * max(1, len(self.sparse_priors)))()
        for i, f in enumerate(self.sparse_priors):
            a = arr[i]
            a.type = int(f["type"]); a.kf = int(f.get("kf", -1)); a.lmk0 = int(f.get("lmk0", -1)); a.lmk1 = int(f.get("lmk1", -1))
            a.kf_b = int(f.get("kf_b", -1))
            for k, n in (("T_prior", 12), ("v_prior", 3), ("ba_prior", 3), ("bg_prior", 3), ("delta", 3)):
                v = np.zeros(n) if f.get(k) is None else np.asarray(f[k], dtype=np.float64).ravel()
                getattr(a, k)[:] = list(v)
            W = np.asarray(f["sqrt_inf"], dtype=np.float64).ravel()
            buf = np.zeros(225); buf[: len(W)] = W
            a.sqrt_inf[:] = list(buf)
        return arr, len(self.sparse_priors)

    def priors_c(self):
        arr = (PosePriorC * max(1, len(self.pose_priors)))()
        for i, (kf, T, inf) in enumerate(self.pose_priors):
            arr[i].kf = int(kf)
            arr[i].T_prior[:] = list(np.asarray(T, dtype=np.float64).ravel())
            arr[i].inf_diag[:] = list(np.asarray(inf, dtype=np.float64).ravel())
        return arr, len(self.pose_priors)

    def imus_c(self):
        arr = (ImuFactorC * max(1, len(self.imu_factors)))()
        for i, f in enumerate(self.imu_factors):
            fill_imu_factor(arr[i], f)
        return arr, len(self.imu_factors)


def sparse_prior_to_dict(s: SparsePriorC) -> dict:
    n = 15 if s.type == SPARSE_IMU_PRIOR else 3
    return {"type": int(s.type), "kf": int(s.kf), "lmk0": int(s.lmk0), "lmk1": int(s.lmk1),
            "T_prior": np.array(s.T_prior[:]), "v_prior": np.array(s.v_prior[:]), "ba_prior": np.array(s.ba_prior[:]),
            "bg_prior": np.array(s.bg_prior[:]), "delta": np.array(s.delta[:]),
            "sqrt_inf": np.array(s.sqrt_inf[: n * n]).reshape(n, n)}


def fill_imu_factor(dst: ImuFactorC, f: dict) -> None:
    dst.kf_i, dst.kf_j, dst.dt = int(f["kf_i"]), int(f["kf_j"]), float(f["dt"])
    for k in ("delta_R", "delta_v", "delta_p", "J_dR_bg", "J_dv_ba", "J_dv_bg", "J_dp_ba", "J_dp_bg", "cov"):
        getattr(dst, k)[:] = list(np.asarray(f[k], dtype=np.float64).ravel())
    dst.bacc_noise, dst.bgyr_noise = float(f["bacc_noise"]), float(f["bgyr_noise"])


class SadvioError(RuntimeError):
    pass


_lib = None


def load_library(path: str = LIB_PATH) -> C.CDLL:
    """Load libsadvio_ba.so. Raises (never falls back) when it is missing."""
    global _lib
    if _lib is not None:
        return _lib
    if not os.path.exists(path):
        raise SadvioError(f"{path} not found: build it with `python -c 'import __graft_entry__ as g; g.build()'` "
                          "(hipcc --offload-arch=gfx950). There is no CPU fallback.")
    lib = C.CDLL(path)
    lib.sadvio_ba_device_count.restype = C.c_int
    lib.sadvio_ba_default_options.argtypes = [C.POINTER(SolveOptions)]
    lib.sadvio_ba_default_options.restype = None
    lib.sadvio_ba_create.argtypes = [C.POINTER(Config), C.POINTER(C.c_void_p)]
    lib.sadvio_ba_destroy.argtypes = [C.c_void_p]
    lib.sadvio_ba_destroy.restype = None
    lib.sadvio_ba_set_windows.argtypes = [C.c_void_p, C.c_int32, C.POINTER(FlatWindowC)]
    lib.sadvio_ba_set_pose_priors.argtypes = [C.c_void_p, C.c_int32, C.c_int32, C.POINTER(PosePriorC)]
    lib.sadvio_ba_set_imu_factors.argtypes = [C.c_void_p, C.c_int32, C.c_int32, C.POINTER(ImuFactorC)]
    lib.sadvio_ba_set_dense_prior.argtypes = [C.c_void_p, C.c_int32, C.c_int32, C.c_int32, _dp, _dp, C.c_int32,
                                              C.c_int32, C.c_int32, _ip, _ip]
    lib.sadvio_ba_set_sparse_priors.argtypes = [C.c_void_p, C.c_int32, C.c_int32, C.POINTER(SparsePriorC)]
    lib.sadvio_ba_marginalize.argtypes = [C.c_void_p, C.c_int32, C.POINTER(MargRequestC), C.POINTER(MargResultC), _ip, _dp, _dp]
    lib.sadvio_ba_sparsify.argtypes = [C.c_void_p, C.c_int32, C.c_int32, C.c_int32, C.c_int32, _dp, C.c_int32, C.c_int32, C.c_int32,
                                        _ip, _ip, _ip, C.POINTER(SparsePriorC)]
    lib.sadvio_ba_set_collective.argtypes = [C.c_void_p, C.c_int32, C.c_int32, ALLREDUCE_FN, C.c_void_p]
    lib.sadvio_ba_rccl_unique_id.argtypes = [C.c_void_p]
    lib.sadvio_ba_comm_init_rccl.argtypes = [C.c_void_p, C.c_int32, C.c_int32, C.c_void_p]
    lib.sadvio_ba_comm_info.argtypes = [C.c_void_p] + [C.POINTER(C.c_int32)] * 4
    lib.sadvio_ba_solve.argtypes = [C.c_void_p, C.POINTER(SolveOptions), C.POINTER(SolveSummary)]
    lib.sadvio_ba_get_deltas.argtypes = [C.c_void_p, C.c_int32, _dp, _dp, _dp, _dp, _dp]
    lib.sadvio_ba_get_ids.argtypes = [C.c_void_p, C.c_int32, _lp, _lp]
    lib.sadvio_ba_get_trace.argtypes = [C.c_void_p, C.c_int32, C.c_int32, _dp, _ip]
    lib.sadvio_ba_set_lines.argtypes = [C.c_void_p, C.c_int32, C.POINTER(LineSetC)]
    lib.sadvio_ba_get_line_deltas.argtypes = [C.c_void_p, C.c_int32, _dp]
    lib.sadvio_ba_marginalize_relative.argtypes = [C.c_void_p, C.c_int32, C.c_int32, C.c_int32, C.c_int32, _dp, _dp]
    if hasattr(lib, "sadvio_ba_marginalize_relative_batch"):   # (an older build loaded through SADVIO_BA_LIB does not export it)
        lib.sadvio_ba_marginalize_relative_batch.argtypes = [C.c_void_p, C.c_int32, C.c_int32, _ip, _ip, C.c_int32, _dp, _dp, _dp, _ip, _ip]
    lib.sadvio_ba_get_prior.argtypes = [C.c_void_p, C.POINTER(PriorInfoC), _dp, _dp]
    lib.sadvio_ba_marg_stats.argtypes = [C.c_void_p, C.POINTER(C.c_int32), C.POINTER(C.c_int32), C.POINTER(C.c_int32)]
    if hasattr(lib, "sadvio_ba_one_round"):
        lib.sadvio_ba_one_round.argtypes = [C.c_void_p, C.POINTER(C.c_int32)]
    lib.sadvio_ba_set_prior.argtypes = [C.c_void_p, C.c_int32, C.c_int32, C.c_int32, _dp, _dp]
    lib.sadvio_ba_linearize.argtypes = [C.c_void_p, C.c_int32, _dp, _dp, _dp, _dp, _dp]
    lib.sadvio_ba_vi_init.argtypes = [C.c_void_p, C.POINTER(ViInitProblemC), C.POINTER(SolveOptions), C.POINTER(SolveSummary),
                                      C.POINTER(ViInitResultC), _dp]
    lib.sadvio_ba_nofov_scale.argtypes = [C.c_void_p, C.POINTER(NoFovProblemC), C.POINTER(SolveOptions), C.POINTER(SolveSummary),
                                          C.POINTER(NoFovResultC), _dp, _dp, _ip]
    if hasattr(lib, "sadvio_ba_covariance"):   # an older build loaded through SADVIO_BA_LIB (A/B measurements) does not export it
        lib.sadvio_ba_covariance.argtypes = [C.c_void_p, C.c_int32, C.POINTER(CovRequestC), _dp, _dp, _dp, _ip]
    if hasattr(lib, "sadvio_ba_covariance_batch"):   # (nor this one)
        lib.sadvio_ba_covariance_batch.argtypes = [C.c_void_p, C.c_int32, C.POINTER(CovBatchItemC)]
    if hasattr(lib, "sadvio_ba_covariance_cross"):   # (nor this one)
        lib.sadvio_ba_covariance_cross.argtypes = [C.c_void_p, C.c_int32, C.POINTER(CovCrossRequestC), _dp, _dp, _dp, _ip]
    lib.sadvio_ba_landmark_chi2.argtypes = [C.c_void_p, C.c_int32, _dp, _dp, _dp, C.c_double, _dp, _ip]
    if hasattr(lib, "sadvio_ba_landmark_chi2_models"):   # (an older build loaded through SADVIO_BA_LIB does not export it)
        lib.sadvio_ba_landmark_chi2_models.argtypes = [C.c_void_p, C.c_int32, _dp, _dp, C.POINTER(CameraModelC), _dp, C.c_double,
                                                       _dp, _ip, _dp]
    lib.sadvio_ba_get_kernel_times.argtypes = [C.c_void_p, C.c_int32, C.POINTER(C.c_char_p), _dp, _lp]
    lib.sadvio_ba_last_error.argtypes = [C.c_void_p]
    lib.sadvio_ba_last_error.restype = C.c_char_p
    lib.sadvio_ba_version.restype = C.c_char_p
    _lib = lib
    return lib


def _ptr(a: Optional[np.ndarray]):
    return a.ctypes.data_as(_dp) if a is not None else _dp()


class Backend:
    """Thin OO wrapper of one `sadvio_ba_handle` (one HIP stream, device-resident windows)."""

    def __init__(self, device: int = 0, profile_kernels: bool = False, use_graph: bool = False, long_tracks: bool = False,
                 long_track_priors: bool = False, long_track_covariance: bool = False, long_track_batch: bool = False):
        """long_tracks: SADVIO_CFG_LONG_TRACKS, the handle accepts landmarks with more than 64 observations.
        long_track_priors: SADVIO_CFG_LONG_TRACK_PRIORS (needs long_tracks), marginalize, sparsify and the prior setters serve them.
        long_track_covariance: SADVIO_CFG_LONG_TRACK_COVARIANCE (needs long_tracks), covariance and covariance_cross serve windows
        that hold them.
        long_track_batch: SADVIO_CFG_LONG_TRACK_BATCH (needs long_tracks), marginalize_relative and marginalize_relative_batch serve
        such windows, and covariance_batch does with long_track_covariance as well."""
        self.lib = load_library()
        flags = ((CFG_LONG_TRACKS if long_tracks else 0) | (CFG_LONG_TRACK_PRIORS if long_track_priors else 0)
                 | (CFG_LONG_TRACK_COVARIANCE if long_track_covariance else 0) | (CFG_LONG_TRACK_BATCH if long_track_batch else 0))
        cfg = Config(device=device, profile_kernels=int(profile_kernels), use_graph=int(use_graph), reserved=flags)
        self.h = C.c_void_p()
        rc = self.lib.sadvio_ba_create(C.byref(cfg), C.byref(self.h))
        if rc == E_INVALID_ARG:
            msg = self.lib.sadvio_ba_last_error(None)
            raise SadvioError(f"sadvio_ba_create failed: rc={rc}: {msg.decode() if msg else ''}")
        if rc != SADVIO_OK:
            raise SadvioError(f"sadvio_ba_create failed: rc={rc} (no gfx950 device? there is no CPU fallback)")
        self.windows: List[FlatWindow] = []

    def _check(self, rc: int, what: str):
        if rc != SADVIO_OK:
            msg = self.lib.sadvio_ba_last_error(self.h)
            raise SadvioError(f"{what} failed: rc={rc}: {msg.decode() if msg else ''}")

    # ---- one window spanning several GPUs (must precede set_windows) ----
    def set_collective(self, rank: int, world: int, fn):
        """fn(ctx, device_ptr, count, hip_stream) -> 0: caller-provided in-place sum all-reduce."""
        self._coll = ALLREDUCE_FN(fn) if fn is not None else ALLREDUCE_FN()
        self._check(self.lib.sadvio_ba_set_collective(self.h, rank, world, self._coll, None), "set_collective")

    def rccl_unique_id(self) -> bytes:
        buf = C.create_string_buffer(RCCL_ID_BYTES)
        self._check(self.lib.sadvio_ba_rccl_unique_id(buf), "rccl_unique_id")
        return buf.raw

    def comm_info(self) -> dict:
        """{nranks, rank, device, is_rccl} of the handle's collective — from the RCCL communicator itself when it is the built-in one."""
        v = [C.c_int32(0) for _ in range(4)]
        self._check(self.lib.sadvio_ba_comm_info(self.h, *[C.byref(x) for x in v]), "comm_info")
        return {"nranks": v[0].value, "rank": v[1].value, "device": v[2].value, "is_rccl": bool(v[3].value)}

    def comm_init_rccl(self, rank: int, world: int, unique_id: bytes):
        assert len(unique_id) == RCCL_ID_BYTES
        self._check(self.lib.sadvio_ba_comm_init_rccl(self.h, rank, world, C.c_char_p(unique_id)), "comm_init_rccl")

    def prepare(self, windows: Sequence[FlatWindow]):
        """Marshal windows (and their factor lists) into the C structs once: what a C++ caller holds anyway. The timed legs
        of bench.py call set_prepared so that Python's per-field conversions stay outside the measurement."""
        prep = {"windows": list(windows), "arr": (FlatWindowC * len(windows))(), "per": []}
        for i, w in enumerate(windows):
            prep["arr"][i] = w.to_c()
            item = {}
            if w.pose_priors:
                item["priors"] = w.priors_c()
            if w.imu_factors:
                item["imus"] = w.imus_c()
            raw = getattr(w, "sparse_raw", None)
            if raw is not None:
                item["sparse"] = raw                      # (SparsePriorC array, n) straight from sparsify(raw=True)
            elif w.sparse_priors:
                item["sparse"] = w.sparse_c()
            prep["per"].append(item)
        return prep

    def set_prepared(self, prep, one_build: bool = True):
        """set_windows + the factor setters of every window; one_build brackets them with begin_update / commit_update (ONE
        layout build and staged upload instead of one per setter)."""
        windows = prep["windows"]
        self.windows = windows
        if one_build:
            self._check(self.lib.sadvio_ba_begin_update(self.h), "begin_update")
            try:
                self._set_prepared(prep)
            except Exception:
                self.lib.sadvio_ba_commit_update(self.h)   # leave the bracket; the error of the setter is the one reported
                raise
            self._check(self.lib.sadvio_ba_commit_update(self.h), "commit_update")
        else:
            self._set_prepared(prep)

    def _set_prepared(self, prep):
        windows = prep["windows"]
        self._check(self.lib.sadvio_ba_set_windows(self.h, len(windows), prep["arr"]), "set_windows")
        for i, w in enumerate(windows):
            item = prep["per"][i]
            if "priors" in item:
                self._check(self.lib.sadvio_ba_set_pose_priors(self.h, i, item["priors"][1], item["priors"][0]), "set_pose_priors")
            if "imus" in item:
                self._check(self.lib.sadvio_ba_set_imu_factors(self.h, i, item["imus"][1], item["imus"][0]), "set_imu_factors")
            if "sparse" in item:
                self._check(self.lib.sadvio_ba_set_sparse_priors(self.h, i, item["sparse"][1], item["sparse"][0]), "set_sparse_priors")
            if w.dense_prior is not None:
                self.set_dense_prior(i, w.dense_prior)
            if w.lines is not None:
                self.set_lines(i, w.lines)

    def set_windows(self, windows: Sequence[FlatWindow], one_build: bool = True):
        self.set_prepared(self.prepare(windows), one_build=one_build)

    def set_lines(self, w: int, lines: Optional[dict]):
        """linexd landmarks of window w (sadvio_ba_set_lines); None clears them."""
        if lines is None:
            self._check(self.lib.sadvio_ba_set_lines(self.h, w, None), "set_lines")
            return
        T = np.ascontiguousarray(lines["T_w_l"], dtype=np.float64).reshape(-1, 12)
        n = T.shape[0]
        c = LineSetC()
        ids = np.ascontiguousarray(lines.get("id", np.arange(n)), dtype=np.int64)
        model = np.ascontiguousarray(lines["model"], dtype=np.float64).reshape(n, 6)
        ptr = np.ascontiguousarray(lines["obs_ptr"], dtype=np.int32)
        okf = np.ascontiguousarray(lines["obs_kf"], dtype=np.int32); ocam = np.ascontiguousarray(lines["obs_cam"], dtype=np.int32)
        meas = np.ascontiguousarray(lines["obs_meas"], dtype=np.float64)
        c.n_line, c.n_obs = n, int(okf.size)
        c.line_id, c.line_T_w_l, c.line_model = ids.ctypes.data_as(_lp), _ptr(T), _ptr(model)
        c.line_obs_ptr, c.obs_kf, c.obs_cam, c.obs_meas = ptr.ctypes.data_as(_ip), okf.ctypes.data_as(_ip), ocam.ctypes.data_as(_ip), _ptr(meas)
        keep = [ids, T, model, ptr, okf, ocam, meas]
        if lines.get("const") is not None:
            lc = np.ascontiguousarray(lines["const"], dtype=np.uint8)
            c.line_const = lc.ctypes.data_as(_bp)
            keep.append(lc)
        self._check(self.lib.sadvio_ba_set_lines(self.h, w, C.byref(c)), "set_lines")

    def get_line_deltas(self, w: int, n_line: int) -> np.ndarray:
        """[n_line, 6] accepted line-pose deltas of window w (PointXYZParametersBlock-style 6-dof blocks of linexd)."""
        out = np.zeros((n_line, 6))
        self._check(self.lib.sadvio_ba_get_line_deltas(self.h, w, _ptr(out)), "get_line_deltas")
        return out

    def set_dense_prior(self, w: int, dp: Optional[dict]):
        """Dense marginalisation prior of window w (None clears it). A dict without "J" (or with resident=True) attaches the
        handle's own prior (SADVIO_PRIOR_RESIDENT): only the kept frame / landmark lists are passed."""
        if dp is None:
            self._check(self.lib.sadvio_ba_set_dense_prior(self.h, w, 0, 0, None, None, -1, 0, 0, None, None), "set_dense_prior")
            return
        li = np.ascontiguousarray(dp.get("lmk_index", []), dtype=np.int32)
        lc = np.ascontiguousarray(dp.get("lmk_col", []), dtype=np.int32)
        if dp.get("resident") or dp.get("J") is None:
            self._check(self.lib.sadvio_ba_set_dense_prior(self.h, w, PRIOR_RESIDENT, 0, None, None, int(dp.get("kf_keep", -1)), int(dp.get("kf_col", 0)),
                                                           len(li), li.ctypes.data_as(_ip), lc.ctypes.data_as(_ip)), "set_dense_prior")
            return
        J = np.ascontiguousarray(dp["J"], dtype=np.float64)
        r0 = np.ascontiguousarray(dp["r0"], dtype=np.float64)
        self._check(self.lib.sadvio_ba_set_dense_prior(self.h, w, J.shape[0], J.shape[1], _ptr(J), _ptr(r0),
                                                       int(dp.get("kf_keep", -1)), int(dp.get("kf_col", 0)), len(li),
                                                       li.ctypes.data_as(_ip), lc.ctypes.data_as(_ip)), "set_dense_prior")

    def marginalize(self, w: int, kf_marg: int, lmk_marg, lmk_keep, kf_keep: int = -1, marg_has_imu: bool = False,
                    imu: Optional[dict] = None, priors=(), last: Optional[dict] = None, eig_cut: str = "noise_floor",
                    form: str = "eigen", readback: bool = True):
        """Dense prior from marginalising key-frame kf_marg of window w (sadvio_ba_marginalize). `last` = previous
        prior as a dense_prior dict (without "J": the handle's resident prior). Returns None when refused (n < 4), else a
        dense_prior dict for the NEXT window (landmark indices still refer to this window) + bookkeeping; with
        readback=False the dict carries no J / r0 (resident=True): the prior only lives on the device."""
        rq = MargRequestC()
        mk = np.ascontiguousarray(lmk_marg, dtype=np.int32); kp = np.ascontiguousarray(lmk_keep, dtype=np.int32)
        rq.kf_marg, rq.kf_keep, rq.marg_has_imu = kf_marg, kf_keep, int(bool(marg_has_imu))
        rq.n_marg, rq.lmk_marg = len(mk), mk.ctypes.data_as(_ip)
        rq.n_keep, rq.lmk_keep = len(kp), kp.ctypes.data_as(_ip)
        rq.eig_cut_mode, rq.prior_form = EIG_CUT[eig_cut], PRIOR_FORM[form]
        keep = [mk, kp]
        if imu is not None:
            ia = (ImuFactorC * 1)()
            fill_imu_factor(ia[0], imu)
            rq.imu = ia
            keep.append(ia)
        pa = (PosePriorC * max(1, len(priors)))()
        for i, (kf, T, inf) in enumerate(priors):
            pa[i].kf = int(kf); pa[i].T_prior[:] = list(np.asarray(T, dtype=np.float64).ravel()); pa[i].inf_diag[:] = list(np.asarray(inf, dtype=np.float64).ravel())
        rq.n_prior, rq.priors = len(priors), pa
        if last is not None:
            li = np.ascontiguousarray(last.get("lmk_index", []), dtype=np.int32); lc = np.ascontiguousarray(last.get("lmk_col", []), dtype=np.int32)
            if last.get("resident") or last.get("J") is None:
                rq.last_n_full, rq.last_n = PRIOR_RESIDENT, 0
            else:
                J = np.ascontiguousarray(last["J"], dtype=np.float64); r0 = np.ascontiguousarray(last["r0"], dtype=np.float64)
                rq.last_n_full, rq.last_n = J.shape
                rq.last_J, rq.last_r0 = _ptr(J), _ptr(r0)
                keep += [J, r0]
            rq.last_kf, rq.last_kf_col = int(last.get("kf_keep", -1)), int(last.get("kf_col", 0))
            rq.last_n_keep, rq.last_lmk_index, rq.last_lmk_col = len(li), li.ctypes.data_as(_ip), lc.ctypes.data_as(_ip)
            keep += [li, lc]
        n = (15 if kf_keep >= 0 else 0) + 3 * len(kp)
        res = MargResultC()
        lmk_col = np.zeros(max(len(kp), 1), dtype=np.int32)
        Jo = np.zeros(max(n * n, 1)) if readback else None
        r0o = np.zeros(max(n, 1)) if readback else None
        rc = self.lib.sadvio_ba_marginalize(self.h, w, C.byref(rq), C.byref(res), lmk_col.ctypes.data_as(_ip), _ptr(Jo), _ptr(r0o))
        if rc == E_REFUSED:
            return None
        self._check(rc, "marginalize")
        nf = res.n_full
        out = {"kf_keep": kf_keep, "kf_col": res.kf_col, "lmk_index": kp.copy(), "lmk_col": lmk_col[: len(kp)].copy(), "m": res.m, "n": res.n,
               "n_full": nf, "sweeps": (res.sweeps_mm, res.sweeps_k), "form": form}
        if readback:
            out["J"] = Jo[: nf * n].reshape(nf, n).copy(); out["r0"] = r0o[:nf].copy()
        else:
            out["resident"] = True
        return out

    def marg_stats(self) -> dict:
        """Route counters of the Cholesky-form marginalisations (sadvio_ba_marg_stats)."""
        v = [C.c_int32(0) for _ in range(3)]
        self._check(self.lib.sadvio_ba_marg_stats(self.h, *[C.byref(x) for x in v]), "marg_stats")
        return {"calls": v[0].value, "unpivoted": v[1].value, "fell_back": v[2].value}

    def one_round(self) -> bool:
        """Whether the last solve ran the single-round instantiations of the tile kernels (sadvio_ba_one_round)."""
        v = C.c_int32()
        self._check(self.lib.sadvio_ba_one_round(self.h, C.byref(v)), "one_round")
        return bool(v.value)

    def get_prior(self, readback: bool = True):
        """The handle's prior (sadvio_ba_get_prior): {"valid", "n_full", "n", "form"[, "J", "r0"]}."""
        info = PriorInfoC()
        self._check(self.lib.sadvio_ba_get_prior(self.h, C.byref(info), None, None), "get_prior")
        out = {"valid": bool(info.valid), "n_full": info.n_full, "n": info.n, "form": "cholesky" if info.form == 1 else "eigen"}
        if info.valid and readback:
            J = np.zeros((info.n_full, info.n)); r0 = np.zeros(info.n_full)
            self._check(self.lib.sadvio_ba_get_prior(self.h, None, _ptr(J), _ptr(r0)), "get_prior")
            out["J"], out["r0"] = J, r0
        return out

    def set_prior(self, J: Optional[np.ndarray], r0: Optional[np.ndarray] = None):
        """Upload an eigen-form prior as the handle's (None clears it)."""
        if J is None:
            self._check(self.lib.sadvio_ba_set_prior(self.h, 0, 0, 0, None, None), "set_prior")
            return
        J = np.ascontiguousarray(J, dtype=np.float64); r0 = np.ascontiguousarray(r0, dtype=np.float64)
        self._check(self.lib.sadvio_ba_set_prior(self.h, J.shape[0], J.shape[1], 0, _ptr(J), _ptr(r0)), "set_prior")

    def marginalize_relative(self, w: int, kf_a: int, kf_b: int, eig_cut: str = "noise_floor"):
        """(inf[6,6], Ak[12,12]) of sadvio_ba_marginalize_relative, or None when refused (no shared landmark)."""
        inf = np.zeros((6, 6)); Ak = np.zeros((12, 12))
        rc = self.lib.sadvio_ba_marginalize_relative(self.h, w, kf_a, kf_b, EIG_CUT[eig_cut], _ptr(inf), _ptr(Ak))
        if rc == E_REFUSED:
            return None
        self._check(rc, "marginalize_relative")
        return inf, Ak

    def marginalize_relative_batch(self, w: int, pairs, eig_cut: str = "noise_floor"):
        """sadvio_ba_marginalize_relative_batch: the relative-pose information of every (kf_a, kf_b) of `pairs` in one call.
        {"inf" [n, 6, 6], "Ak" [n, 12, 12], "T_a_b" [n, 12], "n_shared" [n], "status" [n]}; status[i] is SADVIO_OK or E_REFUSED
        (nothing shared, or a covariance that cannot be inverted: zeros in that pair's outputs)."""
        pr = np.ascontiguousarray(pairs, dtype=np.int32).reshape(-1, 2)
        n = len(pr)
        ka, kb = np.ascontiguousarray(pr[:, 0]), np.ascontiguousarray(pr[:, 1])
        inf = np.zeros((n, 6, 6)); Ak = np.zeros((n, 12, 12)); Tab = np.zeros((n, 12))
        ns = np.zeros(n, dtype=np.int32); st = np.zeros(n, dtype=np.int32)
        rc = self.lib.sadvio_ba_marginalize_relative_batch(self.h, w, n, ka.ctypes.data_as(_ip), kb.ctypes.data_as(_ip), EIG_CUT[eig_cut],
                                                           _ptr(inf), _ptr(Ak), _ptr(Tab), ns.ctypes.data_as(_ip), st.ctypes.data_as(_ip))
        self._check(rc, "marginalize_relative_batch")
        return {"inf": inf, "Ak": Ak, "T_a_b": Tab, "n_shared": ns, "status": st}

    def sparsify(self, w: int, prior: dict, vio: bool, raw: bool = False):
        """NFR sparsification of a dense prior dict (as returned by marginalize; without "J": the handle's resident prior)
        into sparse_priors dicts (raw=True: the (SparsePriorC array, n) pair itself, for FlatWindow.sparse_raw)."""
        li = np.ascontiguousarray(prior.get("lmk_index", []), dtype=np.int32); lc = np.ascontiguousarray(prior.get("lmk_col", []), dtype=np.int32)
        out = (SparsePriorC * (len(li) + 1))()
        n_out = C.c_int32(0)
        if prior.get("resident") or prior.get("J") is None:
            J = None; nf = nn = 0
        else:
            J = np.ascontiguousarray(prior["J"], dtype=np.float64); nf, nn = J.shape
        rc = self.lib.sadvio_ba_sparsify(self.h, w, int(bool(vio)), nf, nn, _ptr(J), int(prior.get("kf_keep", -1)),
                                         int(prior.get("kf_col", 0)), len(li), li.ctypes.data_as(_ip), lc.ctypes.data_as(_ip),
                                         C.byref(n_out), out)
        if rc == E_REFUSED:
            return None
        self._check(rc, "sparsify")
        if raw:
            return out, n_out.value
        return [sparse_prior_to_dict(out[i]) for i in range(n_out.value)]

    def solve(self, opts: Optional[SolveOptions] = None) -> List[SolveSummary]:
        opts = opts or reference_options()
        sums = (SolveSummary * len(self.windows))()
        rc = self.lib.sadvio_ba_solve(self.h, C.byref(opts), sums)
        if rc != E_NOT_USABLE:  # "not usable" (Ceres FAILURE of some window) is reported through summary.termination
            self._check(rc, "solve")
        return list(sums)

    def get_deltas(self, w: int = 0):
        win = self.windows[w]
        pose = np.zeros((win.n_kf, 6)); lmk = np.zeros((win.n_lmk, 3))
        dv = np.zeros((win.n_kf, 3)); dba = np.zeros((win.n_kf, 3)); dbg = np.zeros((win.n_kf, 3))
        self._check(self.lib.sadvio_ba_get_deltas(self.h, w, _ptr(pose), _ptr(lmk), _ptr(dv), _ptr(dba), _ptr(dbg)),
                    "get_deltas")
        return {"pose": pose, "lmk": lmk, "dv": dv, "dba": dba, "dbg": dbg}

    def get_trace(self, w: int = 0) -> np.ndarray:
        """Per-iteration log [iterations + 1, 8] of the last solve (sadvio_ba_get_trace)."""
        n = C.c_int32(0)
        self._check(self.lib.sadvio_ba_get_trace(self.h, w, 0, _dp(), C.byref(n)), "get_trace")
        rows = np.zeros((n.value, 8))
        self._check(self.lib.sadvio_ba_get_trace(self.h, w, n.value, _ptr(rows), C.byref(n)), "get_trace")
        return rows

    def get_ids(self, w: int = 0):
        win = self.windows[w]
        kf = np.zeros(win.n_kf, dtype=np.int64); lm = np.zeros(win.n_lmk, dtype=np.int64)
        self._check(self.lib.sadvio_ba_get_ids(self.h, w, kf.ctypes.data_as(_lp), lm.ctypes.data_as(_lp)), "get_ids")
        return kf, lm

    def linearize(self, w: int = 0, pose_delta=None, lmk_delta=None):
        win = self.windows[w]
        r = np.zeros((win.n_obs, 2)); Jp = np.zeros((win.n_obs, 2, 6)); Jl = np.zeros((win.n_obs, 2, 3))
        pd = None if pose_delta is None else np.ascontiguousarray(pose_delta, dtype=np.float64)
        ld = None if lmk_delta is None else np.ascontiguousarray(lmk_delta, dtype=np.float64)
        self._check(self.lib.sadvio_ba_linearize(self.h, w, _ptr(pd), _ptr(ld), _ptr(r), _ptr(Jp), _ptr(Jl)),
                    "linearize")
        return r, Jp, Jl

    def landmark_chi2(self, w: int = 0, pose_delta=None, lmk_delta=None, image_wh=None, pixel_sigma=0.0):
        """(avg_chi2[n_lmk], inlier[n_lmk]) — ALandmark::sanityCheck (ALandmark.cpp:98-146) at the given deltas."""
        win = self.windows[w]
        avg = np.zeros(win.n_lmk); inl = np.zeros(win.n_lmk, dtype=np.int32)
        pd = None if pose_delta is None else np.ascontiguousarray(pose_delta, dtype=np.float64)
        ld = None if lmk_delta is None else np.ascontiguousarray(lmk_delta, dtype=np.float64)
        wh = None if image_wh is None else np.ascontiguousarray(image_wh, dtype=np.float64)
        self._check(self.lib.sadvio_ba_landmark_chi2(self.h, w, _ptr(pd), _ptr(ld), _ptr(wh), pixel_sigma, _ptr(avg),
                                                     inl.ctypes.data_as(_ip)), "landmark_chi2")
        return avg, inl

    def landmark_chi2_models(self, w: int, models, pose_delta=None, lmk_delta=None, obs_uv=None, pixel_sigma=0.0,
                             want_obs=False, raw_rc=False):
        """(avg_chi2[n_lmk], inlier[n_lmk][, obs_chi2[n_obs]]) — the gate of landmark_chi2 with every observation projected by
        its camera's own model (sadvio_ba_landmark_chi2_models). models: one CameraModelC / dict per camera of window w;
        obs_uv: [n_obs, 2] measured pixels in the window's observation order, or None. raw_rc: the return code comes first and
        nothing raises (outputs are NaN / -1 filled, so that an untouched output shows)."""
        win = self.windows[w] if 0 <= w < len(self.windows) else None
        n_lmk, n_obs = (win.n_lmk, win.n_obs) if win is not None else (0, 0)
        avg = np.full(n_lmk, np.nan) if raw_rc else np.zeros(n_lmk)
        inl = np.full(n_lmk, -1, dtype=np.int32) if raw_rc else np.zeros(n_lmk, dtype=np.int32)
        obs = (np.full(n_obs, np.nan) if raw_rc else np.zeros(n_obs)) if want_obs else None
        pd = None if pose_delta is None else np.ascontiguousarray(pose_delta, dtype=np.float64)
        ld = None if lmk_delta is None else np.ascontiguousarray(lmk_delta, dtype=np.float64)
        uv = None if obs_uv is None else np.ascontiguousarray(obs_uv, dtype=np.float64)
        arr = None if models is None else camera_models_c(models)
        rc = self.lib.sadvio_ba_landmark_chi2_models(self.h, w, _ptr(pd), _ptr(ld), arr, _ptr(uv), pixel_sigma, _ptr(avg),
                                                     inl.ctypes.data_as(_ip), _ptr(obs))
        out = (avg, inl, obs) if want_obs else (avg, inl)
        if raw_rc:
            return (rc,) + out
        self._check(rc, "landmark_chi2_models")
        return out

    def vi_init(self, T_f_w, vel, factors, opts: SolveOptions = None, **kw):
        """AOptimizer::VIInit (AOptimizer.cpp:448-581) on the device; see make_viinit_problem for the arguments."""
        P, keep = make_viinit_problem(T_f_w, vel, factors, **kw)
        s = SolveSummary(); r = ViInitResultC(); dv = np.zeros((P.n_frames, 3))
        rc = self.lib.sadvio_ba_vi_init(self.h, C.byref(P), C.byref(opts or viinit_options()), C.byref(s), C.byref(r), _ptr(dv))
        if rc not in (0, E_NOT_USABLE):
            self._check(rc, "vi_init")
        return viinit_result_to_dict(rc, s, r, dv)

    def nofov_scale(self, opts: SolveOptions = None, raw_rc: bool = False, **kw):
        """AngularAdjustmentCERESAnalytic::landmarkOptimizationNoFov (AngularAdjustmentCERESAnalytic.cpp:741-907) on the device;
        see make_nofov_problem for the arguments. rc SADVIO_E_NOT_USABLE is returned in the dict (the outputs are filled);
        raw_rc=True also returns SADVIO_E_INVALID_ARG there instead of raising."""
        P, keep = make_nofov_problem(**kw)
        n = P.n_lmk
        s = SolveSummary(); r = NoFovResultC()
        dl = np.zeros((n, 3)); gn = np.zeros(n); inl = np.zeros(n, dtype=np.int32)
        rc = self.lib.sadvio_ba_nofov_scale(self.h, C.byref(P), C.byref(opts or nofov_options()), C.byref(s), C.byref(r), _ptr(dl),
                                            _ptr(gn), inl.ctypes.data_as(_ip))
        if rc not in (0, E_NOT_USABLE) and not (raw_rc and rc == E_INVALID_ARG):
            self._check(rc, "nofov_scale")
        return {"rc": rc, "summary": s, "lambda": float(r.lambda_), "usable": bool(r.usable), "scale_fixed": bool(r.scale_fixed),
                "n_inliers": int(r.n_inliers), "lmk_delta": dl, "gate_norm": gn, "inlier": inl}

    def covariance(self, w: int = 0, kf=None, pairs=None, lmk=None, raw_rc: bool = False):
        """Marginal covariances of window w at the last solve's final state (sadvio_ba_covariance).
        kf: key-frame indices -> "kf" [n, d, d] (d = 6, 15 with IMU states); pairs: (a, b) index pairs -> "pair" [n, d, d], the
        cross blocks Sigma(a, b); lmk: landmark indices, or "all" -> "lmk" [n, 3, 3]. "n_lmk_singular": landmarks among them whose
        H_ll is not positive definite (their block is NaN). raw_rc=True returns {"rc", "error"} for a refused call instead of
        raising; the outputs are then untouched (NaN-free zeros as allocated here)."""
        win = self.windows[w] if 0 <= w < len(self.windows) else self.windows[0]   # (an index out of range is the library's to refuse)
        d = 15 if win.has_imu else 6
        rq = CovRequestC()
        ka = np.ascontiguousarray([] if kf is None else kf, dtype=np.int32).reshape(-1)
        pr = np.ascontiguousarray([] if pairs is None else pairs, dtype=np.int32).reshape(-1, 2)
        pa, pb = np.ascontiguousarray(pr[:, 0]), np.ascontiguousarray(pr[:, 1])
        all_lmk = isinstance(lmk, str) and lmk == "all"
        la = np.ascontiguousarray([] if (lmk is None or all_lmk) else lmk, dtype=np.int32).reshape(-1)
        n_l = win.n_lmk if all_lmk else len(la)
        rq.n_kf, rq.kf = len(ka), ka.ctypes.data_as(_ip)
        rq.n_pair, rq.pair_a, rq.pair_b = len(pa), pa.ctypes.data_as(_ip), pb.ctypes.data_as(_ip)
        rq.n_lmk, rq.lmk = (-1 if all_lmk else len(la)), la.ctypes.data_as(_ip)
        kc = np.zeros((len(ka), d, d)); pc = np.zeros((len(pa), d, d)); lc = np.zeros((n_l, 3, 3))
        ns = C.c_int32(0)
        rc = self.lib.sadvio_ba_covariance(self.h, w, C.byref(rq), _ptr(kc) if len(ka) else _dp(), _ptr(pc) if len(pa) else _dp(),
                                           _ptr(lc) if n_l else _dp(), C.byref(ns))
        if rc != SADVIO_OK and raw_rc:
            msg = self.lib.sadvio_ba_last_error(self.h)
            return {"rc": rc, "error": msg.decode() if msg else "", "kf": kc, "pair": pc, "lmk": lc}
        self._check(rc, "covariance")
        return {"rc": rc, "kf": kc, "pair": pc, "lmk": lc, "n_lmk_singular": int(ns.value)}

    def covariance_cross(self, w: int = 0, kf=(), lmk=(), cam=None, meas=None, raw_rc: bool = False, want_innov=None):
        """Cross covariances Sigma(kf[i], lmk[i]) of window w and, with cam / meas (the candidate observation's camera and
        measurement: pixel uv [n, 2] or unit bearing [n, 3]), the innovation covariance and squared Mahalanobis distance of each
        candidate (sadvio_ba_covariance_cross). Returns {"cross" [n, d, 3], "innov" [n, 2, 2], "maha2" [n], "status" [n]} — "innov"
        and "maha2" stay as allocated here (zeros) without cam. raw_rc=True returns {"rc", "error"} plus the untouched outputs for
        a refused call instead of raising. want_innov=True asks for the innovation outputs even without cam (the library refuses)."""
        win = self.windows[w] if 0 <= w < len(self.windows) else self.windows[0]
        d = 15 if win.has_imu else 6
        ka = np.ascontiguousarray(kf, dtype=np.int32).reshape(-1)
        la = np.ascontiguousarray(lmk, dtype=np.int32).reshape(-1)
        n = len(ka)
        if len(la) != n:
            raise ValueError("covariance_cross: kf and lmk differ in length")
        rq = CovCrossRequestC()
        rq.n, rq.kf, rq.lmk = n, ka.ctypes.data_as(_ip), la.ctypes.data_as(_ip)
        ca = ma = None
        if cam is not None:
            ca = np.ascontiguousarray(cam, dtype=np.int32).reshape(-1)
            rq.cam = ca.ctypes.data_as(_ip)
        if meas is not None:
            ma = np.ascontiguousarray(meas, dtype=np.float64).reshape(n, -1)
            rq.meas = _ptr(ma)
        innov = (cam is not None) if want_innov is None else want_innov
        xc = np.zeros((n, d, 3)); pc = np.zeros((n, 2, 2)); m2 = np.zeros(n); st = np.zeros(n, dtype=np.int32)
        rc = self.lib.sadvio_ba_covariance_cross(self.h, w, C.byref(rq), _ptr(xc) if n else _dp(), _ptr(pc) if (n and innov) else _dp(),
                                                 _ptr(m2) if (n and innov) else _dp(), st.ctypes.data_as(_ip) if n else _ip())
        out = {"rc": rc, "cross": xc, "innov": pc, "maha2": m2, "status": st}
        if rc != SADVIO_OK and raw_rc:
            msg = self.lib.sadvio_ba_last_error(self.h)
            out["error"] = msg.decode() if msg else ""
            return out
        self._check(rc, "covariance_cross")
        return out

    def cov_batch_items(self, items, fill: float = 0.0):
        """The sadvio_cov_batch_item array of `items` (dicts w=.., kf=.., pairs=.., lmk=.. with the meanings of covariance()) and the
        output arrays it points to, allocated here and filled with `fill`: (array, one dict of "kf" / "pair" / "lmk" per item, the index
        arrays to keep alive). A caller that repeats a call (scripts/gpu_time_covariance_batch.py) builds them once."""
        arr = (CovBatchItemC * max(len(items), 1))()
        keep, outs = [], []
        for i, it in enumerate(items):
            w = int(it.get("w", 0))
            win = self.windows[w] if 0 <= w < len(self.windows) else self.windows[0]   # (an index out of range is the library's to refuse)
            d = 15 if win.has_imu else 6
            kf, pairs, lmk = it.get("kf"), it.get("pairs"), it.get("lmk")
            ka = np.ascontiguousarray([] if kf is None else kf, dtype=np.int32).reshape(-1)
            pr = np.ascontiguousarray([] if pairs is None else pairs, dtype=np.int32).reshape(-1, 2)
            pa, pb = np.ascontiguousarray(pr[:, 0]), np.ascontiguousarray(pr[:, 1])
            all_lmk = isinstance(lmk, str) and lmk == "all"
            la = np.ascontiguousarray([] if (lmk is None or all_lmk) else lmk, dtype=np.int32).reshape(-1)
            n_l = win.n_lmk if all_lmk else len(la)
            kc = np.full((len(ka), d, d), fill); pc = np.full((len(pa), d, d), fill); lc = np.full((n_l, 3, 3), fill)
            a = arr[i]
            a.w = w
            a.rq.n_kf, a.rq.kf = len(ka), ka.ctypes.data_as(_ip)
            a.rq.n_pair, a.rq.pair_a, a.rq.pair_b = len(pa), pa.ctypes.data_as(_ip), pb.ctypes.data_as(_ip)
            a.rq.n_lmk, a.rq.lmk = (-1 if all_lmk else len(la)), la.ctypes.data_as(_ip)
            a.kf_cov = _ptr(kc) if len(ka) else _dp()
            a.pair_cov = _ptr(pc) if len(pa) else _dp()
            a.lmk_cov = _ptr(lc) if n_l else _dp()
            keep.append((ka, pa, pb, la))
            outs.append({"kf": kc, "pair": pc, "lmk": lc})
        return arr, outs, keep

    def covariance_batch(self, items, raw_rc: bool = False, fill: float = 0.0):
        """Marginal covariances of many windows of the solved batch in one call (sadvio_ba_covariance_batch).
        items: dicts w=.., kf=.., pairs=.., lmk=.. with the meanings of covariance(); a window may appear in several items. Returns
        one dict per item, shaped as covariance() returns, plus "status" (SADVIO_OK | E_NOT_USABLE: that item's outputs are
        untouched) and "route" (COV_ROUTE_*). The outputs are allocated here, filled with `fill`. raw_rc=True returns
        {"rc", "error", "items"} for a refused call instead of raising."""
        n = len(items)
        arr, outs, keep = self.cov_batch_items(items, fill)
        rc = self.lib.sadvio_ba_covariance_batch(self.h, n, arr if n else C.POINTER(CovBatchItemC)())
        if rc == SADVIO_OK:
            for i, o in enumerate(outs):
                o.update(rc=int(arr[i].status), status=int(arr[i].status), route=int(arr[i].route), n_lmk_singular=int(arr[i].n_lmk_singular))
        if rc != SADVIO_OK and raw_rc:
            msg = self.lib.sadvio_ba_last_error(self.h)
            return {"rc": rc, "error": msg.decode() if msg else "", "items": outs}
        self._check(rc, "covariance_batch")
        return outs

    def kernel_times(self):
        cap = 32
        names = (C.c_char_p * cap)(); us = np.zeros(cap); n = np.zeros(cap, dtype=np.int64)
        k = self.lib.sadvio_ba_get_kernel_times(self.h, cap, names, _ptr(us), n.ctypes.data_as(_lp))
        return {names[i].decode(): {"avg_us": float(us[i]), "launches": int(n[i])} for i in range(max(k, 0))}

    def close(self):
        if self.h:
            self.lib.sadvio_ba_destroy(self.h)
            self.h = C.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass
