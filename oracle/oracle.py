"""ctypes wrapper of the CPU oracle — TEST INFRASTRUCTURE ONLY.

Imported only by tests/, __graft_entry__.smoke() and bench.py's cpu_baseline leg (as the checker /
reported baseline, never as the thing shipped). The product path (sadvio_amd/) never imports this.
"""
from __future__ import annotations

import ctypes as C
import os
import subprocess

import numpy as np

from . import structs as S
from .structs import reference_options

# the oracle's own mirrors of the C header (oracle/structs.py) — nothing is imported from the product package
FlatWindowC, ImuFactorC, PosePriorC, SparsePriorC = S.flat_window, S.imu_factor, S.pose_prior, S.sparse_prior
SolveOptions, SolveSummary = S.solve_options, S.solve_summary
fill_imu_factor = S.fill_imu
FlatWindow = object   # any object with the header's field names as attributes (duck-typed)

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB = os.path.join(_HERE, "_build", "libsadvio_oracle.so")
_dp = C.POINTER(C.c_double)
_ip = C.POINTER(C.c_int32)


class OracleProblem(C.Structure):
    _fields_ = [("win", C.POINTER(FlatWindowC)), ("n_prior", C.c_int32), ("priors", C.POINTER(PosePriorC)),
                ("n_imu", C.c_int32), ("imus", C.POINTER(ImuFactorC)),
                ("dp_n_full", C.c_int32), ("dp_n", C.c_int32), ("dp_J", _dp), ("dp_r0", _dp),
                ("dp_kf_keep", C.c_int32), ("dp_kf_col", C.c_int32), ("dp_n_keep", C.c_int32),
                ("dp_lmk_index", _ip), ("dp_lmk_col", _ip), ("n_threads", C.c_int32),
                ("n_sparse", C.c_int32), ("sparse", C.POINTER(SparsePriorC)),
                ("lines", C.POINTER(S.line_set)), ("line_delta6", _dp)]


class ImuState(C.Structure):
    _fields_ = [("acc", C.c_double * 3), ("gyr", C.c_double * 3), ("ba", C.c_double * 3), ("bg", C.c_double * 3),
                ("v", C.c_double * 3), ("T_f_w", C.c_double * 12), ("delta_R", C.c_double * 9),
                ("delta_v", C.c_double * 3), ("delta_p", C.c_double * 3), ("cov", C.c_double * 81),
                ("J_dR_bg", C.c_double * 9), ("J_dv_ba", C.c_double * 9), ("J_dv_bg", C.c_double * 9),
                ("J_dp_ba", C.c_double * 9), ("J_dp_bg", C.c_double * 9), ("ts_ns", C.c_double),
                ("is_keyframe", C.c_int32), ("pad", C.c_int32)]


class MargRequest(C.Structure):
    _fields_ = [("win", C.POINTER(FlatWindowC)), ("kf_marg", C.c_int32), ("kf_keep", C.c_int32),
                ("marg_has_imu", C.c_int32), ("n_marg", C.c_int32), ("lmk_marg", _ip), ("n_keep", C.c_int32),
                ("lmk_keep", _ip), ("imu", C.POINTER(ImuFactorC)), ("n_prior", C.c_int32),
                ("priors", C.POINTER(PosePriorC)), ("last_n_full", C.c_int32), ("last_n", C.c_int32),
                ("last_J", _dp), ("last_r0", _dp), ("last_kf", C.c_int32), ("last_kf_col", C.c_int32),
                ("last_n_keep", C.c_int32), ("last_lmk_index", _ip), ("last_lmk_col", _ip),
                ("eig_cut_mode", C.c_int32), ("pad", C.c_int32)]


EIG_CUT = {"reference": 0, "noise_floor": 1}   # SADVIO_EIG_CUT_* (include/sadvio_ba.h)


class MargResult(C.Structure):
    _fields_ = [("m", C.c_int32), ("n", C.c_int32), ("n_full", C.c_int32), ("kf_col", C.c_int32)]


_lib = None


def build():
    subprocess.run(["make", "-C", _HERE], check=True, capture_output=True)


def lib():
    global _lib
    if _lib is None:
        if not os.path.exists(LIB):
            build()
        _lib = C.CDLL(LIB)
        _lib.oracle_solve.argtypes = [C.POINTER(OracleProblem), C.POINTER(SolveOptions), C.POINTER(SolveSummary),
                                      _dp, _dp, _dp, _dp, _dp, _dp, C.c_int32]
        _lib.oracle_linearize.argtypes = [C.POINTER(FlatWindowC), _dp, _dp, _dp, _dp, _dp, _ip]
        _lib.oracle_viinit.argtypes = [C.POINTER(S.viinit_problem), C.POINTER(SolveOptions), C.POINTER(SolveSummary),
                                       C.POINTER(S.viinit_result), _dp]
        _lib.oracle_factor_imu_init.argtypes = [C.POINTER(ImuFactorC)] + [_dp] * 7
        _lib.oracle_landmark_chi2.argtypes = [C.POINTER(FlatWindowC), _dp, _dp, _dp, C.c_double, _dp, _ip]
        _lib.oracle_first_step.argtypes = [C.POINTER(OracleProblem), C.POINTER(SolveOptions), _dp, _dp, _dp, _dp,
                                           C.c_int32]
        _lib.oracle_imu_process.argtypes = [C.POINTER(ImuState), C.POINTER(ImuState), _dp, _dp, C.c_double,
                                            C.c_double, C.c_double]
        _lib.oracle_imu_bias_correction.argtypes = [C.POINTER(ImuState), _dp, _dp]
        _lib.oracle_factor_imu.argtypes = [C.POINTER(ImuFactorC), _dp, _dp, _dp, _dp, _dp, _dp, _dp]
        _lib.oracle_factor_imu_bias.argtypes = [C.POINTER(ImuFactorC), _dp, _dp, _dp, _dp, _dp, _dp, _dp]
        _lib.oracle_marginalize.argtypes = [C.POINTER(MargRequest), C.POINTER(MargResult), _ip, _dp, _dp, _dp, _dp,
                                            _dp, _dp, _dp, _dp]
        _lib.oracle_marg_information.argtypes = [C.POINTER(MargRequest), C.POINTER(MargResult), _ip, _dp, _dp]
        _lib.oracle_sym_eig.argtypes = [_dp, C.c_int32, _dp, _dp]
    return _lib


def _p(a):
    return a.ctypes.data_as(_dp) if a is not None else _dp()


def _arr(x, n=None):
    a = np.ascontiguousarray(np.asarray(x, dtype=np.float64).ravel())
    assert n is None or a.size == n, (a.size, n)
    return a


def make_problem(w: FlatWindow, dense_prior=None, n_threads=1):
    wc, wkeep = S.window_to_c(w)
    pa, npri = S.priors_to_c(getattr(w, "pose_priors", []))
    ia, nimu = S.imus_to_c(getattr(w, "imu_factors", []))
    P = OracleProblem()
    P.win = C.pointer(wc)
    P.n_prior, P.priors = npri, pa
    P.n_imu, P.imus = nimu, ia
    P.n_threads = n_threads
    sa, nsp = S.sparse_to_c(getattr(w, "sparse_priors", []))
    P.n_sparse, P.sparse = nsp, sa
    keep = [wc, wkeep, pa, ia, sa]
    lines = getattr(w, "lines", None)
    if lines is not None:
        lc, lkeep = S.lines_to_c(lines)
        P.lines = C.pointer(lc)
        keep += [lc, lkeep]
    if dense_prior is not None:
        J = np.ascontiguousarray(dense_prior["J"], dtype=np.float64)
        r0 = np.ascontiguousarray(dense_prior["r0"], dtype=np.float64)
        li = np.ascontiguousarray(dense_prior["lmk_index"], dtype=np.int32)
        lc = np.ascontiguousarray(dense_prior["lmk_col"], dtype=np.int32)
        P.dp_n_full, P.dp_n = J.shape
        P.dp_J, P.dp_r0 = _p(J), _p(r0)
        P.dp_kf_keep, P.dp_kf_col = int(dense_prior.get("kf_keep", -1)), int(dense_prior.get("kf_col", 0))
        P.dp_n_keep = len(li)
        P.dp_lmk_index, P.dp_lmk_col = li.ctypes.data_as(_ip), lc.ctypes.data_as(_ip)
        keep += [J, r0, li, lc]
    return P, keep


def solve(w: FlatWindow, opts: SolveOptions = None, dense_prior=None, n_threads=1, log_cap=64):
    opts = S.options_from(opts)
    P, keep = make_problem(w, dense_prior, n_threads)
    pose = np.zeros((w.n_kf, 6)); lmk = np.zeros((w.n_lmk, 3))
    dv = np.zeros((w.n_kf, 3)); dba = np.zeros((w.n_kf, 3)); dbg = np.zeros((w.n_kf, 3))
    log = np.zeros((log_cap, 8))
    s = SolveSummary()
    line = None
    if getattr(w, "lines", None) is not None:
        line = np.zeros((np.asarray(w.lines["T_w_l"]).reshape(-1, 12).shape[0], 6))
        P.line_delta6 = _p(line)
    rc = lib().oracle_solve(C.byref(P), C.byref(opts), C.byref(s), _p(pose), _p(lmk), _p(dv), _p(dba), _p(dbg),
                            _p(log), log_cap)
    return {"rc": rc, "summary": s, "pose": pose, "lmk": lmk, "dv": dv, "dba": dba, "dbg": dbg, "line": line,
            "log": log[: s.iterations + 1]}


def line_factor(w, l: int, o: int, xp=None, xline=None):
    """(r, J[rows, 12]) of line observation o of line l at the given deltas: columns [key-frame 6 | line 6]."""
    wc, wkeep = S.window_to_c(w)
    lc, lkeep = S.lines_to_c(w.lines)
    r = np.zeros(4); J = np.zeros((4, 12))
    a = None if xp is None else np.ascontiguousarray(xp, dtype=np.float64)
    b = None if xline is None else np.ascontiguousarray(xline, dtype=np.float64)
    f = lib().oracle_line_factor
    f.argtypes = [C.c_void_p, C.c_void_p, C.c_int32, C.c_int32, _dp, _dp, _dp, _dp]
    rows = f(C.byref(wc), C.byref(lc), l, o, _p(a), _p(b), _p(r), _p(J))
    return r[:rows].copy(), J[:rows].copy()


def linearize(w: FlatWindow, pose_delta=None, lmk_delta=None):
    wc, wkeep = S.window_to_c(w)
    r = np.zeros((w.n_obs, 2)); Jp = np.zeros((w.n_obs, 2, 6)); Jl = np.zeros((w.n_obs, 2, 3))
    valid = np.zeros(w.n_obs, dtype=np.int32)
    pd = None if pose_delta is None else _arr(pose_delta, 6 * w.n_kf)
    ld = None if lmk_delta is None else _arr(lmk_delta, 3 * w.n_lmk)
    lib().oracle_linearize(C.byref(wc), _p(pd), _p(ld), _p(r), _p(Jp), _p(Jl), valid.ctypes.data_as(_ip))
    return r, Jp, Jl, valid


def landmark_chi2(w: FlatWindow, pose_delta=None, lmk_delta=None, image_wh=None, pixel_sigma=0.0):
    """(avg_chi2[n_lmk], inlier[n_lmk]) — ALandmark::sanityCheck at the given deltas."""
    wc, wkeep = S.window_to_c(w)
    avg = np.zeros(w.n_lmk); inl = np.zeros(w.n_lmk, dtype=np.int32)
    pd = None if pose_delta is None else _arr(pose_delta, 6 * w.n_kf)
    ld = None if lmk_delta is None else _arr(lmk_delta, 3 * w.n_lmk)
    wh = None if image_wh is None else _arr(image_wh, 2 * w.n_cam)
    rc = lib().oracle_landmark_chi2(C.byref(wc), _p(pd), _p(ld), _p(wh), pixel_sigma, _p(avg), inl.ctypes.data_as(_ip))
    assert rc == 0, rc
    return avg, inl


def first_step(w: FlatWindow, opts: SolveOptions = None):
    """(delta_pose, delta_lmk, H_full, g_full) of the first LM step at zero deltas."""
    opts = S.options_from(opts)
    P, keep = make_problem(w)
    dp = np.zeros((w.n_kf, 6)); dl = np.zeros((w.n_lmk, 3))
    N = lib().oracle_first_step(C.byref(P), C.byref(opts), _dp(), _dp(), _p(np.zeros(1)), _p(np.zeros(1)), -1)
    H = np.zeros((N, N)); g = np.zeros(N)
    rc = lib().oracle_first_step(C.byref(P), C.byref(opts), _p(dp), _p(dl), _p(H), _p(g), N)
    assert rc == 0, rc
    return dp, dl, H, g


def sparse_factor(w: FlatWindow, k: int, xp=None, xv=None, xba=None, xbg=None, xl=None):
    """(r[rows], J[rows,15]) of sparse prior factor k of the window at the given deltas."""
    wc, wkeep = S.window_to_c(w)
    sa, _ = S.sparse_to_c(w.sparse_priors)
    r = np.zeros(15); J = np.zeros((15, 15))
    arrs = [None if a is None else np.ascontiguousarray(a, dtype=np.float64) for a in (xp, xv, xba, xbg, xl)]
    f = lib().oracle_sparse_factor
    f.argtypes = [C.c_void_p, C.c_void_p] + [_dp] * 7
    rows = f(C.byref(wc), C.byref(sa[k]), *[_p(a) for a in arrs], _p(r), _p(J))
    return r[:rows].copy(), J[:rows].copy()


def marginalize(w: FlatWindow, kf_marg, lmk_marg, lmk_keep, kf_keep=-1, marg_has_imu=False, imu=None, priors=(), last=None, want_full=False,
                eig_cut="noise_floor"):
    """oracle_marginalize with the same calling convention as capi.Backend.marginalize. Returns None when refused.
    want_full: also return A_full [(m+n)^2], b_full [m+n] (the un-reduced information / gradient, computeInformationAndGradient)."""
    rq, keep, kp, mk = _marg_request(w, kf_marg, lmk_marg, lmk_keep, kf_keep, marg_has_imu, imu, priors, last, eig_cut)
    n = (15 if kf_keep >= 0 else 0) + 3 * len(kp)
    res = MargResult()
    lmk_col = np.zeros(max(len(kp), 1), dtype=np.int32); Jo = np.zeros(max(n * n, 1)); r0o = np.zeros(max(n, 1))
    Ak = np.zeros((max(n, 1), max(n, 1))); bk = np.zeros(max(n, 1))
    m_max = (15 if marg_has_imu else 6) + 3 * len(mk)
    Af = np.zeros((m_max + n) ** 2) if want_full else None
    bf = np.zeros(m_max + n) if want_full else None
    rc = lib().oracle_marginalize(C.byref(rq), C.byref(res), lmk_col.ctypes.data_as(_ip), _p(Af) if want_full else _dp(), _p(bf) if want_full else _dp(),
                                  _p(Ak), _p(bk), _dp(), _dp(), _p(Jo), _p(r0o))
    if rc != 0:
        return None
    nf = res.n_full
    extra = {}
    if want_full:
        N = res.m + res.n
        extra = {"A_full": Af[: N * N].reshape(N, N).copy(), "b_full": bf[:N].copy()}
    return {**extra, "J": Jo[: nf * n].reshape(nf, n).copy(), "r0": r0o[:nf].copy(), "kf_keep": kf_keep, "kf_col": res.kf_col,
            "lmk_index": kp.copy(), "lmk_col": lmk_col[: len(kp)].copy(), "m": res.m, "n": res.n, "n_full": nf, "Ak": Ak, "bk": bk}


def marg_information(w: FlatWindow, kf_marg, lmk_marg, lmk_keep, kf_keep=-1, marg_has_imu=False, imu=None, priors=(), last=None):
    """oracle_marg_information: marginalize()'s A_full [(m+n)^2] / b_full [m+n] and index layout (m, n, kf_col, lmk_col),
    without the Schur complement and eigen-decompositions. Returns None when refused (n < 4)."""
    rq, keep, kp, mk = _marg_request(w, kf_marg, lmk_marg, lmk_keep, kf_keep, marg_has_imu, imu, priors, last, "noise_floor")
    n = (15 if kf_keep >= 0 else 0) + 3 * len(kp)
    N = (15 if marg_has_imu else 6) + 3 * len(mk) + n
    res = MargResult()
    lmk_col = np.zeros(max(len(kp), 1), dtype=np.int32)
    Af = np.zeros((N, N)); bf = np.zeros(N)
    rc = lib().oracle_marg_information(C.byref(rq), C.byref(res), lmk_col.ctypes.data_as(_ip), _p(Af), _p(bf))
    if rc != 0:
        return None
    assert res.m + res.n == N
    return {"A_full": Af, "b_full": bf, "m": res.m, "n": res.n, "kf_keep": kf_keep, "kf_col": res.kf_col, "lmk_index": kp.copy(),
            "lmk_col": lmk_col[: len(kp)].copy()}


def _marg_request(w, kf_marg, lmk_marg, lmk_keep, kf_keep, marg_has_imu, imu, priors, last, eig_cut):
    """The oracle_marg_request of marginalize() / marg_information() and the arrays it points into (keep them alive)."""
    wc, wkeep = S.window_to_c(w)
    rq = MargRequest()
    rq.win = C.pointer(wc)
    mk = np.ascontiguousarray(lmk_marg, dtype=np.int32); kp = np.ascontiguousarray(lmk_keep, dtype=np.int32)
    rq.kf_marg, rq.kf_keep, rq.marg_has_imu = kf_marg, kf_keep, int(bool(marg_has_imu))
    rq.n_marg, rq.lmk_marg = len(mk), mk.ctypes.data_as(_ip)
    rq.n_keep, rq.lmk_keep = len(kp), kp.ctypes.data_as(_ip)
    rq.eig_cut_mode = EIG_CUT[eig_cut]
    keep = [wc, wkeep, mk, kp]
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
        J = np.ascontiguousarray(last["J"], dtype=np.float64); r0 = np.ascontiguousarray(last["r0"], dtype=np.float64)
        li = np.ascontiguousarray(last.get("lmk_index", []), dtype=np.int32); lc = np.ascontiguousarray(last.get("lmk_col", []), dtype=np.int32)
        rq.last_n_full, rq.last_n = J.shape
        rq.last_J, rq.last_r0 = _p(J), _p(r0)
        rq.last_kf, rq.last_kf_col = int(last.get("kf_keep", -1)), int(last.get("kf_col", 0))
        rq.last_n_keep, rq.last_lmk_index, rq.last_lmk_col = len(li), li.ctypes.data_as(_ip), lc.ctypes.data_as(_ip)
        keep += [J, r0, li, lc]
    return rq, keep, kp, mk


def marginalize_relative(w: FlatWindow, kf_a: int, kf_b: int, eig_cut="noise_floor"):
    """(inf[6,6], Ak[12,12], m) of oracle_marginalize_relative, or None when no landmark is shared."""
    wc, wkeep = S.window_to_c(w)
    inf = np.zeros((6, 6)); Ak = np.zeros((12, 12)); m = C.c_int32(0)
    f = lib().oracle_marginalize_relative
    f.argtypes = [C.c_void_p, C.c_int32, C.c_int32, C.c_int32, _dp, _dp, C.POINTER(C.c_int32)]
    rc = f(C.byref(wc), kf_a, kf_b, EIG_CUT[eig_cut], _p(inf), _p(Ak), C.byref(m))
    if rc != 0:
        return None
    return inf, Ak, m.value


def sparsify(w: FlatWindow, prior: dict, vio: bool):
    """oracle_sparsify: dense prior dict -> list of sparse prior dicts (None when refused)."""
    wc, wkeep = S.window_to_c(w)
    J = np.ascontiguousarray(prior["J"], dtype=np.float64)
    li = np.ascontiguousarray(prior.get("lmk_index", []), dtype=np.int32); lc = np.ascontiguousarray(prior.get("lmk_col", []), dtype=np.int32)
    out = (SparsePriorC * (len(li) + 1))()
    n_out = C.c_int32(0)
    f = lib().oracle_sparsify
    f.argtypes = [C.c_void_p, C.c_int32, C.c_int32, C.c_int32, _dp, C.c_int32, C.c_int32, C.c_int32, _ip, _ip, _ip, C.c_void_p]
    rc = f(C.byref(wc), int(bool(vio)), J.shape[0], J.shape[1], _p(J), int(prior.get("kf_keep", -1)), int(prior.get("kf_col", 0)), len(li),
           li.ctypes.data_as(_ip), lc.ctypes.data_as(_ip), C.byref(n_out), out)
    if rc != 0:
        return None
    return [_sparse_to_dict(out[i]) for i in range(n_out.value)]


def _sparse_to_dict(s):
    n = 15 if s.type == 0 else (6 if s.type == 4 else 3)
    return {"type": int(s.type), "kf": int(s.kf), "kf_b": int(s.kf_b), "lmk0": int(s.lmk0), "lmk1": int(s.lmk1),
            "T_prior": np.array(s.T_prior[:]), "v_prior": np.array(s.v_prior[:]), "ba_prior": np.array(s.ba_prior[:]),
            "bg_prior": np.array(s.bg_prior[:]), "delta": np.array(s.delta[:]),
            "sqrt_inf": np.array(s.sqrt_inf[: n * n]).reshape(n, n)}


# ---- factor probes ----
def factor_pixel(T0, K, Tsf, p0, uv, sigma, dpose, dl):
    r = np.zeros(2); Jp = np.zeros((2, 6)); Jl = np.zeros((2, 3)); v = C.c_int32(0)
    f = lib().oracle_factor_pixel
    f.argtypes = [_dp] * 5 + [C.c_double] + [_dp] * 5 + [C.POINTER(C.c_int32)]
    f(_p(_arr(T0, 12)), _p(_arr(K, 4)), _p(_arr(Tsf, 12)), _p(_arr(p0, 3)), _p(_arr(uv, 2)), float(sigma),
      _p(_arr(dpose, 6)), _p(_arr(dl, 3)), _p(r), _p(Jp), _p(Jl), C.byref(v))
    return r, Jp, Jl, v.value


def factor_angular(T0, Tsf, p0, b, sigma, dpose, dl):
    r = np.zeros(2); Jp = np.zeros((2, 6)); Jl = np.zeros((2, 3))
    f = lib().oracle_factor_angular
    f.argtypes = [_dp] * 4 + [C.c_double] + [_dp] * 5
    f(_p(_arr(T0, 12)), _p(_arr(Tsf, 12)), _p(_arr(p0, 3)), _p(_arr(b, 3)), float(sigma), _p(_arr(dpose, 6)),
      _p(_arr(dl, 3)), _p(r), _p(Jp), _p(Jl))
    return r, Jp, Jl


def factor_pose_prior(T0, Tprior, inf_diag, dpose):
    r = np.zeros(6); J = np.zeros((6, 6))
    f = lib().oracle_factor_pose_prior
    f.argtypes = [_dp] * 6
    f(_p(_arr(T0, 12)), _p(_arr(Tprior, 12)), _p(_arr(inf_diag, 6)), _p(_arr(dpose, 6)), _p(r), _p(J))
    return r, J


def factor_imu(fdict, Ti0, Tj0, vi0, vj0, params24):
    fc = ImuFactorC()
    fill_imu_factor(fc, fdict)
    r = np.zeros(9); J = np.zeros((9, 24))
    rc = lib().oracle_factor_imu(C.byref(fc), _p(_arr(Ti0, 12)), _p(_arr(Tj0, 12)), _p(_arr(vi0, 3)),
                                 _p(_arr(vj0, 3)), _p(_arr(params24, 24)), _p(r), _p(J))
    assert rc == 0, rc
    return r, J


def factor_imu_init(fdict, Ti, Tj, vi, vj, params15):
    """IMUFactorInit (residuals.hpp:302-410): (r[9], J[9,15]) with columns r_wi(2) dv_i(3) dv_j(3) dba(3) dbg(3) lambda."""
    fc = ImuFactorC()
    fill_imu_factor(fc, fdict)
    r = np.zeros(9); J = np.zeros((9, 15))
    rc = lib().oracle_factor_imu_init(C.byref(fc), _p(_arr(Ti, 12)), _p(_arr(Tj, 12)), _p(_arr(vi, 3)), _p(_arr(vj, 3)),
                                      _p(_arr(params15, 15)), _p(r), _p(J))
    assert rc == 0, rc
    return r, J


def viinit(T_f_w, vel, factors, opts=None, **kw):
    """AOptimizer::VIInit (AOptimizer.cpp:448-581) restated; arguments as capi.make_viinit_problem."""
    T = np.ascontiguousarray(T_f_w, dtype=np.float64).reshape(-1, 12)
    v = np.ascontiguousarray(vel, dtype=np.float64).reshape(-1, 3)
    arr, nf = S.imus_to_c(factors)
    P = S.viinit_problem(T.shape[0], nf, T.ctypes.data_as(_dp), v.ctypes.data_as(_dp), arr, int(kw.get("optim_scale", False)),
                         int(kw.get("optim_bias", False)), float(kw.get("sigma_dba", 1.0)), float(kw.get("sigma_dbg", 1.0)))
    o = S.options_from(opts)
    if opts is None:
        o.max_num_iterations = 50   # AOptimizer.cpp:518-528
    s = SolveSummary(); r = S.viinit_result(); dv = np.zeros((P.n_frames, 3))
    rc = lib().oracle_viinit(C.byref(P), C.byref(o), C.byref(s), C.byref(r), _p(dv))
    return {"rc": rc, "summary": s, "r_wi": np.array(r.r_wi[:]), "lambda": float(r.lambda_), "dba": np.array(r.dba[:]),
            "dbg": np.array(r.dbg[:]), "R_w_i": np.array(r.R_w_i[:]).reshape(3, 3), "scale": float(r.scale), "dv": dv}


def factor_imu_bias(fdict, bai, bgi, baj, bgj, params12):
    fc = ImuFactorC()
    fill_imu_factor(fc, fdict)
    r = np.zeros(6); J = np.zeros((6, 12))
    lib().oracle_factor_imu_bias(C.byref(fc), _p(_arr(bai, 3)), _p(_arr(bgi, 3)), _p(_arr(baj, 3)), _p(_arr(bgj, 3)),
                                 _p(_arr(params12, 12)), _p(r), _p(J))
    return r, J


def so3_exp(w):
    R = np.zeros((3, 3)); f = lib().oracle_so3_exp; f.argtypes = [_dp, _dp]; f(_p(_arr(w, 3)), _p(R)); return R


def so3_log(R):
    w = np.zeros(3); f = lib().oracle_so3_log; f.argtypes = [_dp, _dp]; f(_p(_arr(R, 9)), _p(w)); return w


def so3_right_jacobian(w):
    J = np.zeros((3, 3)); f = lib().oracle_so3_right_jacobian; f.argtypes = [_dp, _dp]; f(_p(_arr(w, 3)), _p(J))
    return J


# ---- IMU pre-integration helpers ----
def new_imu_state(acc, gyr, ts_ns, T_f_w=None, keyframe=False, ba=(0, 0, 0), bg=(0, 0, 0), v=(0, 0, 0)) -> ImuState:
    s = ImuState()
    s.acc[:] = list(acc); s.gyr[:] = list(gyr)
    s.ba[:] = list(ba); s.bg[:] = list(bg); s.v[:] = list(v)
    T = np.concatenate([np.eye(3).ravel(), np.zeros(3)]) if T_f_w is None else np.asarray(T_f_w, dtype=np.float64)
    s.T_f_w[:] = list(T)
    s.delta_R[:] = list(np.eye(3).ravel())  # IMU.h:36 (config constructor)
    s.ts_ns = float(ts_ns)
    s.is_keyframe = int(keyframe)
    return s


def imu_process(cur: ImuState, last: ImuState, kf: ImuState, gyr_noise, acc_noise, rate_hz) -> bool:
    kb = _arr(list(kf.ba)); kg = _arr(list(kf.bg))
    return bool(lib().oracle_imu_process(C.byref(cur), C.byref(last), _p(kb), _p(kg), gyr_noise, acc_noise, rate_hz))


def imu_factor_dict(kf_i, kf_j, last: ImuState, dt, bacc_noise, bgyr_noise) -> dict:
    g = lambda name: np.array(list(getattr(last, name)))
    return {"kf_i": kf_i, "kf_j": kf_j, "dt": dt, "delta_R": g("delta_R"), "delta_v": g("delta_v"),
            "delta_p": g("delta_p"), "J_dR_bg": g("J_dR_bg"), "J_dv_ba": g("J_dv_ba"), "J_dv_bg": g("J_dv_bg"),
            "J_dp_ba": g("J_dp_ba"), "J_dp_bg": g("J_dp_bg"), "cov": g("cov"), "bacc_noise": bacc_noise,
            "bgyr_noise": bgyr_noise}


def sym_eig(A):
    A = np.ascontiguousarray(A, dtype=np.float64)
    n = A.shape[0]
    ev = np.zeros(n); V = np.zeros((n, n))
    lib().oracle_sym_eig(_p(A), n, _p(ev), _p(V))
    return ev, V
