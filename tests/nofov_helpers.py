"""CPU reference of the NoFov scale solve (AngularAdjustmentCERESAnalytic::landmarkOptimizationNoFov,
AngularAdjustmentCERESAnalytic.cpp:741-907) and a generator of its problems.

  * scale_factor: AngularErrorScaleCam0::Evaluate (AngularAdjustmentCERESAnalytic.h:131-189) on oracle.twin's scalar back ends,
    composing the transforms as the reference does (T_cam_w = T_cam_cam0 * T_cam0_cam0p(lambda)^-1 * T_cam0_w);
  * NoFovProblem: the whole problem for twin.lm_solve(problem=...) (dense, any back end: small problems and 50-digit runs).
    twin.lm_solve starts every parameter at 0, so x[0] is lambda - 1 there; its x_norm therefore omits lambda's 1, which only
    moves the parameter-tolerance test (never reached by the problems compared with it);
  * arrowhead_lm: vectorised float64 LM with the same Ceres-2.2 schedule on the arrowhead normal equations, Ceres' x_norm
    (lambda's value included), for problems of thousands of landmarks;
  * make_nofov: scaleTest's rig (tests/golden/nofov_isae_bench.json) with seeded points, noise, outliers and extra key-frames.
Problems are dicts with the keyword arguments of sadvio_amd.capi.make_nofov_problem (+ "truth")."""
import json
import os

import numpy as np

from oracle import twin

HERE = os.path.dirname(os.path.abspath(__file__))
FIXTURE = os.path.join(HERE, "golden", "nofov_isae_bench.json")
HUBER_A = 1.345 ** 0.5
DEFAULTS = dict(twin.DEFAULTS, huber_a=HUBER_A)


def fixture():
    with open(FIXTURE) as f:
        d = json.load(f)
    for k in ("T_f_s1", "T_f_s2", "T_f_fp"):
        M = np.array(d[k], dtype=np.float64)
        U, _, Vt = np.linalg.svd(M[:3, :3])                          # the printed rotations carry 6-8 digits: nearest rotation,
        M[:3, :3] = U @ Vt                                           # so that an inverse is the transpose (the factors assume it)
        d[k] = M
    return d


def T12(M):
    return np.concatenate([M[:3, :3].ravel(), M[:3, 3]])


def M4(T):
    T = np.asarray(T, dtype=np.float64).reshape(12)
    M = np.eye(4)
    M[:3, :3] = T[:9].reshape(3, 3); M[:3, 3] = T[9:]
    return M


def inv4(M):
    R, t = M[:3, :3], M[:3, 3]
    out = np.eye(4)
    out[:3, :3] = R.T; out[:3, 3] = -R.T @ t
    return out


def log_so3_norm(R):
    return float(np.linalg.norm(twin.log_so3(twin.Backend("f64"), np.asarray(R, dtype=np.float64))))


def reference_fix_scale(T_cam0_cam0p):
    """:769-772"""
    M = M4(T_cam0_cam0p)
    return log_so3_norm(M[:3, :3]) < 0.05 or np.linalg.norm(M[:3, 3]) < 0.01


# ------------------------------------------------------------------------------------------------------------------------------
# AngularErrorScaleCam0
# ------------------------------------------------------------------------------------------------------------------------------
def _basis(B, b):
    ex = np.array([B.s(1), B.s(0), B.s(0)], dtype=B.dtype)
    ez = np.array([B.s(0), B.s(0), B.s(1)], dtype=B.dtype)
    cross = lambda u, v: np.array([u[1] * v[2] - u[2] * v[1], u[2] * v[0] - u[0] * v[2], u[0] * v[1] - u[1] * v[0]], dtype=B.dtype)
    b1 = cross(b, ex) if twin.norm(B, b - ex) > 1e-5 else cross(b, ez)
    b1 = b1 / twin.norm(B, b1)
    b2 = cross(b1, b)
    return np.stack([b1, b2 / twin.norm(B, b2)])


def scale_factor(B, bearing, p0, T_cam0_w, T_cam0_cam0p, T_cam_cam0, sigma, lam, dl):
    """AngularErrorScaleCam0::Evaluate. Returns r[2], J_lambda[2], J_lmk[2, 3]. Transforms are 12-vectors."""
    Rw, tw = twin.split_T(B, T_cam0_w)
    Rm, tm = twin.split_T(B, T_cam0_cam0p)
    Rc, tc = twin.split_T(B, T_cam_cam0)
    b = B.a(bearing)
    q = B.a(p0) + B.a(dl)                                        # :137
    w = 1 / (B.s(sigma) * B.s(sigma))                            # :138, 1 / sigma^2
    ts = lam * tm                                                # :141-142
    R_inv, t_inv = Rm.T, -(Rm.T @ ts)
    R_cw = Rc @ R_inv @ Rw                                       # :143
    t_cw = Rc @ (R_inv @ tw + t_inv) + tc
    tsl = R_cw @ q + t_cw                                        # :146
    nrm = twin.norm(B, tsl)
    bs = tsl / nrm
    Pt = _basis(B, b)                                            # :150-162
    r = w * (Pt @ (bs - b))                                      # :165
    Je = Pt @ (B.eye(3) - np.outer(bs, bs)) / nrm                # :169-170
    J_lam = w * (Je @ (-(Rc @ Rm.T @ tm)))                       # :175-177
    J_l = w * (Je @ (Rc @ Rm.T @ Rw))                            # :182-184
    return r, J_lam, J_l


def _tables(pb):
    """T_cam0_w and T_cam_cam0 of every camera as 12-vectors (:808-813)."""
    Tf = M4(np.asarray(pb["frame_T_f_w"]).reshape(-1, 12)[0])
    Ts = [M4(t) for t in np.asarray(pb["cam_T_s_f"]).reshape(-1, 12)]
    c0 = int(pb.get("cam0", 0))
    T_cam0_w = T12(Ts[c0] @ Tf)
    T_cc0 = [T12(T @ inv4(Ts[c0])) for T in Ts]
    return T_cam0_w, T_cc0


def is_fixed(pb):
    fs = int(pb.get("fix_scale", -1))
    return reference_fix_scale(pb["T_cam0_cam0p"]) if fs < 0 else bool(fs)


class NoFovProblem:
    """The problem of landmarkOptimizationNoFov for twin.lm_solve(problem=...): x = [lambda - 1 (unless lambda is constant),
    dl_0, dl_1, ...]; rows of a landmark: the scale factor, then its fixed-pose angular factors; the scale prior last."""

    def __init__(self, B, pb, huber_a=HUBER_A):
        self.B, self.pb, self.huber_a = B, pb, float(huber_a)
        self.fixed = is_fixed(pb)
        self.lp = np.asarray(pb["lmk_p"], dtype=np.float64).reshape(-1, 3)
        self.n_lmk = self.lp.shape[0]
        self.c_lam = -1 if self.fixed else 0
        self.c0 = 0 if self.fixed else 1
        self.n = self.c0 + 3 * self.n_lmk
        self.T_cam0_w, self.T_cc0 = _tables(pb)
        self.has_imu = False

    def unpack(self, x):
        lam = self.B.s(1) + (x[0] if not self.fixed else self.B.s(0))
        return lam, [x[self.c0 + 3 * l: self.c0 + 3 * l + 3] for l in range(self.n_lmk)]

    def blocks(self, x):
        """(r, [(col, J)], loss) per residual block, before the loss."""
        B, pb = self.B, self.pb
        lam, dls = self.unpack(x)
        Tf = np.asarray(pb["frame_T_f_w"]).reshape(-1, 12); Ts = np.asarray(pb["cam_T_s_f"]).reshape(-1, 12)
        ptr = pb["lmk_obs_ptr"]
        for l in range(self.n_lmk):
            c = self.c0 + 3 * l
            r, Jlam, Jl = scale_factor(B, pb["scale_bearing"][l], self.lp[l], self.T_cam0_w, pb["T_cam0_cam0p"],
                                       self.T_cc0[int(pb["scale_cam"][l])], 1.0, lam, dls[l])
            cols = [(c, Jl)] + ([(0, Jlam.reshape(2, 1))] if not self.fixed else [])
            yield r, cols, True
            for o in range(int(ptr[l]), int(ptr[l + 1])):
                r, _, Jl = twin.angular_factor(B, Tf[int(pb["obs_frame"][o])], Ts[int(pb["obs_cam"][o])], self.lp[l],
                                               pb["obs_bearing"][o], 1.0, np.zeros(6), dls[l])
                yield r, [(c, Jl)], True
        if not self.fixed:                                           # scalePrior: r = info (1 - lambda), no loss
            info = B.s(float(pb.get("info_scale", 0.0)))
            yield np.array([info * (1 - lam)], dtype=B.dtype), [(0, np.array([[-info]], dtype=B.dtype))], False

    def evaluate(self, x, want_j=True):
        B = self.B
        rs, rows, cost = [], [], B.s(0)
        for r, cols, loss in self.blocks(x):
            s = sum(v * v for v in r)
            rho = s
            if loss and self.huber_a > 0:                            # corrector.cc, rho'' <= 0: r and J scaled by sqrt(rho')
                rho, d1 = twin.huber(B, s, self.huber_a)
                sc = B.sqrt(d1)
                r = sc * r
                cols = [(c, sc * J) for c, J in cols]
            cost = cost + rho / 2
            rs.append(r); rows.append(cols)
        res = np.concatenate(rs) if rs else B.zeros(0)
        if not want_j:
            return cost, B.s(0), res, None
        J = B.zeros((len(res), self.n))
        i = 0
        for r, cols in zip(rs, rows):
            for c, Jb in cols:
                J[i: i + len(r), c: c + Jb.shape[1]] = Jb
            i += len(r)
        return cost, B.s(0), res, J


def twin_solve(pb, opts=None, kind="f64", digits=50, huber_a=HUBER_A):
    """twin.lm_solve on NoFovProblem; returns the summary fields, lambda and the landmark deltas."""
    P = NoFovProblem(twin.Backend(kind, digits), pb, huber_a)
    out = twin.lm_solve(None, opts=dict(DEFAULTS, **(opts or {})), problem=P)
    x = out["x_scalar"]
    lam, dls = P.unpack(x)
    out["lambda"] = float(lam)
    out["lmk_delta"] = np.array([[float(v) for v in d] for d in dls]).reshape(-1, 3)
    return out


# ------------------------------------------------------------------------------------------------------------------------------
# vectorised float64 arrowhead LM
# ------------------------------------------------------------------------------------------------------------------------------
def _basis_v(b):
    ex = np.array([1.0, 0.0, 0.0]); ez = np.array([0.0, 0.0, 1.0])
    far = np.linalg.norm(b - ex, axis=1) > 1e-5
    b1 = np.where(far[:, None], np.cross(b, ex), np.cross(b, ez))
    b1 /= np.linalg.norm(b1, axis=1)[:, None]
    b2 = np.cross(b1, b)
    b2 /= np.linalg.norm(b2, axis=1)[:, None]
    return np.stack([b1, b2], axis=1)                                # [n, 2, 3]


def _bearing_v(tsl, b, R):
    """r [n, 2] and Je [n, 2, 3] (= Pt (I - bs bs^T) / |t| R) of bearing residuals."""
    nrm = np.linalg.norm(tsl, axis=1)
    bs = tsl / nrm[:, None]
    Pt = _basis_v(b)
    r = np.einsum("nij,nj->ni", Pt, bs - b)
    Pr = (Pt - np.einsum("nij,nj->ni", Pt, bs)[:, :, None] * bs[:, None, :]) / nrm[:, None, None]
    return r, Pr if R is None else np.einsum("nij,njk->nik", Pr, R)


def _huber_v(s, a):
    if a <= 0:
        return s, np.ones_like(s)
    out = s <= a * a
    rr = np.sqrt(s)
    rho = np.where(out, s, 2 * a * rr - a * a)
    sc = np.where(out, 1.0, np.sqrt(np.maximum(a / np.where(out, 1.0, rr), np.finfo(np.float64).tiny)))
    return rho, sc


class Arrowhead:
    def __init__(self, pb, huber_a=HUBER_A):
        self.pb, self.a = pb, float(huber_a)
        self.fixed = is_fixed(pb)
        self.lp = np.asarray(pb["lmk_p"], dtype=np.float64).reshape(-1, 3)
        self.n = self.lp.shape[0]
        self.sb = np.asarray(pb["scale_bearing"], dtype=np.float64).reshape(-1, 3)
        self.sc = np.asarray(pb["scale_cam"], dtype=int).reshape(-1)
        ptr = np.asarray(pb["lmk_obs_ptr"], dtype=int)
        self.olmk = np.repeat(np.arange(self.n), np.diff(ptr)) if self.n else np.zeros(0, dtype=int)
        Tf = np.asarray(pb["frame_T_f_w"]).reshape(-1, 12); Ts = np.asarray(pb["cam_T_s_f"]).reshape(-1, 12)
        of = np.asarray(pb["obs_frame"], dtype=int).reshape(-1); oc = np.asarray(pb["obs_cam"], dtype=int).reshape(-1)
        Msf = np.array([M4(Ts[c]) @ M4(Tf[k]) for k, c in zip(of, oc)]).reshape(-1, 4, 4)   # T_s_f * T_f_w (:62)
        self.oR, self.ot = Msf[:, :3, :3], Msf[:, :3, 3]
        self.ob = np.asarray(pb["obs_bearing"], dtype=np.float64).reshape(-1, 3)
        T_cam0_w, T_cc0 = _tables(pb)
        self.Mw, self.Mm = M4(T_cam0_w), M4(pb["T_cam0_cam0p"])
        self.Mc = [M4(t) for t in T_cc0]
        self.info = float(pb.get("info_scale", 0.0))

    def scale_rows(self, lam, dl, huber=True):
        """r [n, 2], J_lambda [n, 2], J_l [n, 3] (loss-corrected when huber), rho [n]."""
        Rm, tm = self.Mm[:3, :3], self.Mm[:3, 3]
        Minv = np.eye(4); Minv[:3, :3] = Rm.T; Minv[:3, 3] = -Rm.T @ (lam * tm)
        R = np.zeros((self.n, 3, 3)); t = np.zeros((self.n, 3)); V = np.zeros((self.n, 3)); A = np.zeros((self.n, 3, 3))
        for c in np.unique(self.sc):
            Mc = self.Mc[c]
            M = Mc @ Minv @ self.Mw
            k = self.sc == c
            R[k], t[k] = M[:3, :3], M[:3, 3]
            V[k] = -(Mc[:3, :3] @ Rm.T @ tm)
            A[k] = Mc[:3, :3] @ Rm.T @ self.Mw[:3, :3]
        tsl = np.einsum("nij,nj->ni", R, self.lp + dl) + t
        r, Pr = _bearing_v(tsl, self.sb, None)
        Jlam = np.einsum("nij,nj->ni", Pr, V)
        Jl = np.einsum("nij,njk->nik", Pr, A)
        s = (r * r).sum(1)
        rho, sc = _huber_v(s, self.a) if huber else (s, np.ones_like(s))
        return r * sc[:, None], Jlam * sc[:, None], Jl * sc[:, None, None], rho

    def obs_rows(self, dl):
        q = self.lp[self.olmk] + dl[self.olmk]
        tsl = np.einsum("nij,nj->ni", self.oR, q) + self.ot
        r, Jl = _bearing_v(tsl, self.ob, self.oR)
        s = (r * r).sum(1)
        rho, sc = _huber_v(s, self.a)
        return r * sc[:, None], Jl * sc[:, None, None], rho

    def linearize(self, lam, dl):
        """cost, H_ll [n,3,3], g_l [n,3], c_l [n,3], H_lamlam, g_lam."""
        r, Jlam, Jl, rho = self.scale_rows(lam, dl)
        H = np.einsum("nqi,nqj->nij", Jl, Jl); g = np.einsum("nqi,nq->ni", Jl, r)
        c = np.einsum("nqi,nq->ni", Jl, Jlam)
        hl = (Jlam * Jlam).sum(); gl = (Jlam * r).sum()
        cost = rho.sum()
        if len(self.olmk):
            ro, Jo, rho_o = self.obs_rows(dl)
            np.add.at(H, self.olmk, np.einsum("nqi,nqj->nij", Jo, Jo))
            np.add.at(g, self.olmk, np.einsum("nqi,nq->ni", Jo, ro))
            cost += rho_o.sum()
        rp = self.info * (1.0 - lam)
        if not self.fixed:
            cost += rp * rp
        return 0.5 * cost, H, g, c, hl + self.info ** 2, gl - self.info * rp

    def cost(self, lam, dl):
        return self.linearize(lam, dl)[0]


def arrowhead_lm(pb, opts=None, huber_a=HUBER_A):
    """The device's algorithm in float64 numpy: returns summary fields, lambda, the landmark deltas, the gate norms."""
    o = dict(DEFAULTS, **(opts or {}))
    A = Arrowhead(pb, huber_a)
    n, fixed = A.n, A.fixed
    lam, x = 1.0, np.zeros((n, 3))
    x_norm = 0.0 if fixed else 1.0
    cost, H, g, c, hl, gl = A.linearize(lam, x)
    dg = lambda M: np.stack([M[:, 0, 0], M[:, 1, 1], M[:, 2, 2]], axis=1)
    sc = 1.0 / (1.0 + np.sqrt(dg(H))) if o["jacobi_scaling"] else np.ones((n, 3))
    sl = 1.0 / (1.0 + np.sqrt(hl)) if o["jacobi_scaling"] else 1.0
    gmax = lambda g, gl: max(np.abs(g).max() if n else 0.0, 0.0 if fixed else abs(gl))
    gm = gmax(g, gl)
    out = dict(initial_cost=cost, n_success=0, n_unsuccess=0, termination=0)
    radius, dec = o["initial_trust_region_radius"], 2.0
    it = n_invalid = 0
    while True:
        if it >= o["max_num_iterations"]:
            out["termination"] = 0; break
        if gm <= o["gradient_tolerance"]:
            out["termination"] = 3; break
        if radius < o["min_trust_region_radius"]:
            out["termination"] = 4; break
        it += 1
        s2 = sc * sc
        M = H.copy()
        for i in range(3):
            M[:, i, i] += np.minimum(np.maximum(s2[:, i] * H[:, i, i], o["min_lm_diagonal"]), o["max_lm_diagonal"]) / radius / s2[:, i]
        ok = True
        try:
            L = np.linalg.cholesky(M) if n else M
        except np.linalg.LinAlgError:
            ok = False
        y_lam = 0.0
        if ok and not fixed:
            Mi_c = np.linalg.solve(M, c[:, :, None])[:, :, 0] if n else c
            S = hl + min(max(sl * sl * hl, o["min_lm_diagonal"]), o["max_lm_diagonal"]) / radius / (sl * sl) - (c * Mi_c).sum()
            y_lam = (gl - (Mi_c * g).sum()) / S
            ok = S > 0 and np.isfinite(y_lam)
        mcc = 0.0
        if ok:
            y = np.linalg.solve(M, (g - c * y_lam)[:, :, None])[:, :, 0] if n else np.zeros((0, 3))
            d, dl_ = -y, -y_lam
            ok = bool(np.isfinite(d).all())
            mcc = -((d * (g + 0.5 * np.einsum("nij,nj->ni", H, d) + dl_ * c)).sum() + dl_ * (gl + 0.5 * hl * dl_))
        if not ok or not mcc > 0:
            n_invalid += 1; out["n_unsuccess"] += 1
            if n_invalid >= o["max_num_consecutive_invalid_steps"]:
                out["termination"] = 5; break
            radius *= 0.5
            continue
        n_invalid = 0
        lam_c = lam + (0.0 if fixed else dl_)
        xc = x + d
        step_norm = np.sqrt((d * d).sum() + dl_ * dl_)
        cc = A.linearize(lam_c, xc)
        cost_change = cost - cc[0]
        if step_norm <= o["parameter_tolerance"] * (x_norm + o["parameter_tolerance"]):
            out["termination"] = 2; break
        if abs(cost_change) <= o["function_tolerance"] * cost:
            out["termination"] = 1; break
        rho = cost_change / mcc
        if rho > o["min_relative_decrease"]:
            lam, x = lam_c, xc
            x_norm = np.sqrt((x * x).sum() + (0.0 if fixed else lam * lam))
            cost, H, g, c, hl, gl = cc
            gm = gmax(g, gl)
            radius = min(o["max_trust_region_radius"], radius / max(1.0 / 3.0, 1.0 - (2.0 * rho - 1.0) ** 3))
            dec = 2.0
            out["n_success"] += 1
        else:
            radius /= dec; dec *= 2.0
            out["n_unsuccess"] += 1
    r, _, _, _ = A.scale_rows(lam, x, huber=False)
    gate_norm = np.sqrt((r * r).sum(1))
    out.update(iterations=it, final_cost=cost, final_radius=radius, **{"lambda": lam}, lmk_delta=x, gate_norm=gate_norm,
               inlier=(~(gate_norm > float(pb.get("gate", 0.02)))).astype(np.int32), scale_fixed=fixed)
    out["usable"] = out["termination"] != 5 and 0.5 <= lam <= 1.5
    return out


# ------------------------------------------------------------------------------------------------------------------------------
# scaleTest's problem, generalised
# ------------------------------------------------------------------------------------------------------------------------------
def _project(Mcw, K, wh, p):
    """pinhole Camera::project: (ok, u, v); ok = depth >= 0.1 and inside the image (Camera.cpp:26-52)."""
    q = Mcw[:3, :3] @ p + Mcw[:3, 3]
    if q[2] < 0.1:
        return False, 0.0, 0.0
    u = K["fx"] * q[0] / q[2] + K["cx"]; v = K["fy"] * q[1] / q[2] + K["cy"]
    return (0 <= u <= wh[0] and 0 <= v <= wh[1]), u, v


def _ray(K, u, v):
    b = np.array([(u - K["cx"]) / K["fx"], (v - K["cy"]) / K["fy"], 1.0])
    return b / np.linalg.norm(b)


def make_nofov(seed=0, n_points=10000, scale0=1.2, px_noise=0.0, lmk_noise=0.0, n_outliers=0, n_extra=0, info_scale=0.0,
               motion=None, fix_scale=-1, max_lmk=None):
    """scaleTest (nofov_test.cpp:59-191): f at the origin, fp at T_f_fp, the ISAE-bench rig, points uniform in a 10 m box; a point
    seen by sensor 1 in both frames, else by sensor 2 in both, becomes a landmark (feat on f, featp on fp, same sensor). Extra
    key-frames (random motions of f) add fixed-pose factors (`feats`); T_cam0_cam0p starts from the truth's translation * scale0."""
    fx = fixture()
    rng = np.random.default_rng(seed)
    K, wh = fx["K"], fx["image_wh"]
    T_f_s = [fx["T_f_s1"], fx["T_f_s2"]]
    T_s_f = [inv4(T) for T in T_f_s]
    T_f_fp = fx["T_f_fp"] if motion is None else motion
    frames = [np.eye(4)]                                               # T_f_w of f; fp: T_f_w = T_f_fp^-1
    Tfp = inv4(T_f_fp)
    for k in range(n_extra):
        w = rng.normal(0, 0.05, 3); t = rng.normal(0, 0.3, 3)
        M = np.eye(4)
        M[:3, :3] = twin.exp_so3(twin.Backend("f64"), w); M[:3, 3] = t
        frames.append(inv4(M))                                         # T_f_w of an extra key-frame
    truth = inv4(T_f_s[0]) @ T_f_fp @ T_f_s[0]                         # T_s1_s1p
    Tm = truth.copy(); Tm[:3, 3] *= scale0
    lp, sb, scam, ptr, of, oc, ob, ptrue = [], [], [], [0], [], [], [], []
    box = fx["point_box"]
    for _ in range(n_points):
        p = box * rng.uniform(-1, 1, 3)
        for c in (0, 1):
            ok, u, v = _project(T_s_f[c] @ frames[0], K, wh, p)
            okp, up, vp = _project(T_s_f[c] @ Tfp, K, wh, p)
            if ok and okp:
                break
        else:
            continue
        nz = lambda: rng.normal(0, px_noise, 2) if px_noise > 0 else np.zeros(2)
        e, ep = nz(), nz()
        ptrue.append(p)
        lp.append(p + (rng.normal(0, lmk_noise, 3) if lmk_noise > 0 else 0.0))
        sb.append(_ray(K, up + ep[0], vp + ep[1])); scam.append(c)
        of.append(0); oc.append(c); ob.append(_ray(K, u + e[0], v + e[1]))   # feat on f
        for k in range(1, len(frames)):
            for cc in (0, 1):
                okk, uk, vk = _project(T_s_f[cc] @ frames[k], K, wh, p)
                if okk and len(of) - ptr[-1] < 16:
                    e = nz()
                    of.append(k); oc.append(cc); ob.append(_ray(K, uk + e[0], vk + e[1]))
        ptr.append(len(of))
        if max_lmk is not None and len(lp) >= max_lmk:
            break
    n = len(lp)
    sb = np.array(sb).reshape(-1, 3)
    out_idx = rng.choice(n, size=min(n_outliers, n), replace=False) if n_outliers else np.zeros(0, dtype=int)
    for l in out_idx:                                                  # planted: featp's bearing rotated by ~3-6 degrees
        w = rng.normal(0, 1, 3); w *= rng.uniform(0.05, 0.1) / np.linalg.norm(w)
        sb[l] = twin.exp_so3(twin.Backend("f64"), w) @ sb[l]
    return dict(frame_T_f_w=np.array([T12(M) for M in frames]), cam_T_s_f=np.array([T12(T) for T in T_s_f]), T_cam0_cam0p=T12(Tm),
                lmk_p=np.array(lp).reshape(-1, 3), scale_bearing=sb, scale_cam=np.array(scam, dtype=np.int32),
                lmk_obs_ptr=np.array(ptr, dtype=np.int32), obs_frame=np.array(of, dtype=np.int32), obs_cam=np.array(oc, dtype=np.int32),
                obs_bearing=np.array(ob).reshape(-1, 3), cam0=0, fix_scale=fix_scale, info_scale=info_scale,
                gate=2.0 / ((K["fx"] + K["fy"]) / 2), truth=T12(truth), lmk_true=np.array(ptrue).reshape(-1, 3), outliers=out_idx)


def abi(pb):
    """The keyword arguments of capi.make_nofov_problem."""
    return {k: v for k, v in pb.items() if k not in ("truth", "lmk_true", "outliers")}
