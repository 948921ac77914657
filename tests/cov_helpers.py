"""Reference for sadvio_ba_covariance (test infrastructure): the FULL information matrix of a window at a given state and blocks of
its plain inverse.

information(w, deltas, huber_a) builds H = J^T J over (free key-frame states + 3 x free landmarks) in float64 from the Jacobians of
oracle/twin.py's Problem (every residual block of the window: visual factors under the Huber corrector, PosePriordx, IMUFactor +
IMUBiasFactor, the five sparse-prior factor types, the dense prior), evaluated at the linearisation origin composed with `deltas`.
reference_blocks() returns blocks of np.linalg.inv(H) of the WHOLE matrix: no Schur complement, so a comparison with the device also
checks the elimination algebra. A free landmark with fewer than two observations that no prior factor touches has a rank-deficient
H_ll: the library leaves it and its observation out of H and reports NaN, and so does this helper.

mp_blocks() is the 50-digit yardstick (mpmath): the same blocks of the inverse of the same float64 matrix. Small matrices go through
mpmath's general inverse; with hundreds of landmarks that is hours of Python, so the landmarks that couple to no other landmark are
eliminated block-wise in 50-digit arithmetic (exact algebra, not an approximation; tests/test_cov_cpu.py checks the two routes
against each other on the small windows and the block route's residual H X = I on the large ones).

E_REF[case] = the largest relative block difference between the float64 inverse and the 50-digit one on that window, measured by
tests/test_cov_cpu.py at the oracle's solution and recorded here rounded up; a device block passes at TOL_FACTOR x E_REF."""
import dataclasses

import numpy as np

from oracle import twin
from sadvio_amd import capi, synthetic

TOL_FACTOR = 64.0
HUBER_A = 1.345 ** 0.5
SINGLE = 7   # the landmark of the pixel VO window that keeps one observation

# float64 yardsticks (see the module docstring); measured by test_cov_cpu.py::test_float64_inverse_against_50_digits
E_REF = {
    "pixel_vo": 2.4e-12,
    "angular_vo": 7.5e-13,
    "huber": 2.4e-12,
    "vio_dense": 1.3e-9,
    "vio_sparse": 1.2e-9,
    "obs64": 8.3e-12,
    "lmk600": 7.4e-13,
}


# ---- windows -------------------------------------------------------------------------------------------------------------------
def _keep_observations(w, keep):
    """w with only the observations whose mask entry is set."""
    keep = np.asarray(keep, dtype=bool)
    cnt = np.array([keep[w.lmk_obs_ptr[l]:w.lmk_obs_ptr[l + 1]].sum() for l in range(w.n_lmk)])
    ptr = np.concatenate([[0], np.cumsum(cnt)]).astype(np.int32)
    return dataclasses.replace(w, lmk_obs_ptr=ptr, obs_kf=w.obs_kf[keep].copy(), obs_cam=w.obs_cam[keep].copy(), obs_meas=w.obs_meas[keep].copy())


def window_pixel_vo():
    """3 KF x 40 landmarks x 2 cameras, the oldest key-frame constant and carrying its pose prior: N_p = 12. Landmark SINGLE keeps one
    observation."""
    w = synthetic.make_window(n_kf=3, n_lmk=40, obs_per_lmk=4, seed=101)
    keep = np.ones(w.n_obs, dtype=bool)
    keep[w.lmk_obs_ptr[SINGLE] + 1:w.lmk_obs_ptr[SINGLE + 1]] = False
    return _keep_observations(w, keep)


def window_angular_vo():
    """4 KF, angular factor: N_p = 18 crosses the 16-column tile of the dense factorisation."""
    return synthetic.make_window(n_kf=4, n_lmk=40, obs_per_lmk=4, seed=102, factor=capi.FACTOR_ANGULAR)


def window_huber():
    """The pixel VO window with three gross outliers (solved under HuberLoss(sqrt(1.345)))."""
    w = window_pixel_vo()
    meas = w.obs_meas.copy()
    for o, d in ((5, (60.0, -45.0)), (50, (-80.0, 30.0)), (100, (40.0, 70.0))):
        meas[o] += d
    w.obs_meas = meas
    return w


def _assemble(base, picks):
    """base's key-frames and cameras with the landmarks picks: (window, landmark, observation positions or None)."""
    lmk_p, ptr, kf, cam, meas = [], [0], [], [], []
    for src, l, sel in picks:
        o = np.arange(src.lmk_obs_ptr[l], src.lmk_obs_ptr[l + 1])
        if sel is not None:
            o = o[sel]
        lmk_p.append(src.lmk_p[l]); kf.append(src.obs_kf[o]); cam.append(src.obs_cam[o]); meas.append(src.obs_meas[o])
        ptr.append(ptr[-1] + len(o))
    return capi.FlatWindow(
        kf_T_f_w=base.kf_T_f_w, kf_const=base.kf_const, cam_K=base.cam_K, cam_T_s_f=base.cam_T_s_f, cam_sigma=base.cam_sigma,
        lmk_p=np.array(lmk_p), lmk_obs_ptr=np.array(ptr, dtype=np.int32), obs_kf=np.concatenate(kf).astype(np.int32),
        obs_cam=np.concatenate(cam).astype(np.int32), obs_meas=np.concatenate(meas), factor_type=base.factor_type, has_imu=0,
        kf_id=base.kf_id, lmk_id=(500000 + 7 * np.arange(len(picks))).astype(np.int64), pose_priors=list(base.pose_priors))


def window_obs64():
    """A 32-KF stereo window (31 free key-frames) of 200 tracks of 10 observations and, between them, one landmark seen by all 64
    views: the per-landmark gather of k_cov_lmk at its widest. The key-frames stand 13 cm apart so that one point is in every view."""
    kw = dict(n_kf=32, seed=105, length=4.0)
    a = synthetic.make_window(n_lmk=200, obs_per_lmk=10, **kw)
    b = synthetic.make_window(n_lmk=1, obs_per_lmk=64, **kw)
    assert np.array_equal(a.kf_T_f_w[a.kf_const == 1], b.kf_T_f_w[b.kf_const == 1])   # same trajectory
    return _assemble(a, [(a, l, None) for l in range(100)] + [(b, 0, None)] + [(a, l, None) for l in range(100, 200)])


OBS64_LMK = 100   # its index in window_obs64()


def window_lmk600():
    """600 narrow tracks over 8 key-frames with five set-aside outlier tracks between them (as tests/test_gpu_tile_packing.py's
    "outliers" window): several landmark tiles."""
    a = synthetic.make_window(n_kf=8, n_lmk=600, seed=11)
    b = synthetic.make_window(n_kf=8, n_lmk=96, obs_per_lmk=12, seed=11)
    assert np.array_equal(a.kf_T_f_w[a.kf_const == 1], b.kf_T_f_w[b.kf_const == 1])
    wide = []
    for j in range(b.n_lmk):
        k = b.obs_kf[b.lmk_obs_ptr[j]:b.lmk_obs_ptr[j + 1]]
        first = [i for i in range(len(k)) if i == 0 or k[i] != k[i - 1]]
        if len(first) >= 5 and 1 <= k[first[:5]].min() and k[first[:5]].max() <= 5:
            wide.append((b, j, np.array(first[:5])))
    assert len(wide) >= 5
    at = {10: wide[0:1], 120: wide[1:2], 300: wide[2:4], 450: wide[4:5]}
    picks = []
    for l in range(a.n_lmk):
        picks += at.get(l, [])
        picks.append((a, l, None))
    return _assemble(a, picks)


VIO_J0 = np.diag(np.concatenate([10.0 * np.ones(6), 5.0 * np.ones(3), 20.0 * np.ones(3), 50.0 * np.ones(3)]))
VIO_N_KEEP = 5


def vio_marg_step():
    """The first step of the per-key-frame loop of tests/test_gpu_sliding.py on a 5-KF VIO window: (w, args, w2, keep) — the window
    whose oldest key-frame is marginalised, the arguments of marginalize (without `last`'s arrays: the initial prior VIO_J0 on the
    oldest frame's 15 states is the caller's to attach), the 4-KF window solved next (three IMU pairs, nothing constant) and the
    VIO_N_KEEP landmarks the prior keeps."""
    from test_gpu_sliding import sub_window
    from vio_helpers import make_vio_window
    W = make_vio_window(n_kf=5, n_lmk=120, seed=141, obs_per_lmk=6)
    state = {"T": W.kf_T_f_w.copy(), "p": W.lmk_p.copy(), "v": W.kf_vel.copy(), "ba": W.kf_ba.copy(), "bg": W.kf_bg.copy()}
    kfs = list(range(5))
    frame0, frame1 = 4, 3
    w, _ = sub_window(W, state, kfs)
    w.pose_priors = [(frame0, W.truth["T_f_w"][frame0].copy(), 100.0 * np.ones(6))]
    keep, marg = synthetic.pre_marginalize(w, frame0)
    keep = keep[:VIO_N_KEEP]
    assert len(keep) == VIO_N_KEEP
    imu = [f for f in w.imu_factors if f["kf_i"] == frame0 and f["kf_j"] == frame1][0]
    last = {"kf_keep": frame0, "kf_col": 0, "lmk_index": np.zeros(0, dtype=np.int32), "lmk_col": np.zeros(0, dtype=np.int32)}
    args = dict(kf_marg=frame0, lmk_marg=marg, lmk_keep=keep, kf_keep=frame1, marg_has_imu=True, imu=imu, priors=w.pose_priors, last=last,
                eig_cut="reference")
    w2, _ = sub_window(W, state, kfs[:-1])
    return w, args, w2, keep


def vio_attach(w, w2, keep, g, sparse):
    """w2 with the prior g (a marginalize result on w, holding J / r0) attached as the dense prior, or with its sparsified factors."""
    w2 = dataclasses.replace(w2)
    if sparse is not None:
        remap = []
        for f in sparse:
            f = dict(f)
            if f["kf"] >= 0:
                f["kf"] = int(np.flatnonzero(w2.kf_id == w.kf_id[f["kf"]])[0])
            if f["lmk0"] >= 0:
                j = np.flatnonzero(w2.lmk_id == w.lmk_id[f["lmk0"]])
                if not len(j):
                    continue
                f["lmk0"] = int(j[0])
            remap.append(f)
        w2.sparse_priors = remap
        return w2
    idx, col = [], []
    for l, lc in zip(keep, g["lmk_col"]):
        j = np.flatnonzero(w2.lmk_id == w.lmk_id[l])
        idx.append(int(j[0]) if len(j) else 0); col.append(int(lc) if len(j) else -1)
    w2.dense_prior = {"kf_keep": int(np.flatnonzero(w2.kf_id == w.kf_id[g["kf_keep"]])[0]), "kf_col": g["kf_col"],
                      "lmk_index": np.array(idx, dtype=np.int32), "lmk_col": np.array(col, dtype=np.int32), "J": g["J"], "r0": g["r0"]}
    return w2


# ---- the information matrix and blocks of its inverse ---------------------------------------------------------------------------
def singular_landmarks(w):
    """Free landmarks with fewer than two observations that no prior factor touches."""
    touched = set()
    for f in (getattr(w, "sparse_priors", None) or []):
        for key in ("lmk0", "lmk1"):
            if int(f.get(key, -1)) >= 0:
                touched.add(int(f[key]))
    dp = getattr(w, "dense_prior", None)
    if dp is not None:
        touched |= {int(li) for li, lc in zip(dp["lmk_index"], dp["lmk_col"]) if lc >= 0}
    lc = np.zeros(w.n_lmk, bool) if w.lmk_const is None else np.asarray(w.lmk_const).astype(bool)
    n = np.diff(w.lmk_obs_ptr)
    return [l for l in range(w.n_lmk) if not lc[l] and n[l] < 2 and l not in touched]


class Information:
    """H of a window at a state, with the index set of every key-frame and landmark block."""

    def __init__(self, w, deltas, huber_a=0.0):
        self.w = w
        self.singular = singular_landmarks(w)
        keep = np.ones(w.n_obs, dtype=bool)
        for l in self.singular:
            keep[w.lmk_obs_ptr[l]:w.lmk_obs_ptr[l + 1]] = False
        wr = _keep_observations(w, keep) if self.singular else w
        B = twin.Backend("f64")
        P = twin.Problem(B, wr, huber_a)
        x = np.zeros(P.n)
        for k in range(w.n_kf):
            if P.kf_col[k] >= 0:
                x[P.kf_col[k]:P.kf_col[k] + 6] = deltas["pose"][k]
                if P.has_imu:
                    x[P.v_col[k]:P.v_col[k] + 3] = deltas["dv"][k]; x[P.ba_col[k]:P.ba_col[k] + 3] = deltas["dba"][k]
                    x[P.bg_col[k]:P.bg_col[k] + 3] = deltas["dbg"][k]
        for l in range(w.n_lmk):
            if P.lmk_col[l] >= 0:
                x[P.lmk_col[l]:P.lmk_col[l] + 3] = deltas["lmk"][l]
        _, _, _, J = P.evaluate(x)
        self.H = J.T @ J
        self.n = P.n
        self.d = 15 if P.has_imu else 6
        self.kf_idx, self.lmk_idx = [], []
        for k in range(w.n_kf):
            if P.kf_col[k] < 0:
                self.kf_idx.append(None)
                continue
            idx = list(range(P.kf_col[k], P.kf_col[k] + 6))
            if P.has_imu:
                for c in (P.v_col[k], P.ba_col[k], P.bg_col[k]):
                    idx += list(range(c, c + 3))
            self.kf_idx.append(np.array(idx))
        for l in range(w.n_lmk):
            self.lmk_idx.append(np.arange(P.lmk_col[l], P.lmk_col[l] + 3) if P.lmk_col[l] >= 0 else None)

    def blocks_of(self, X):
        """{"kf" [n_kf, d, d], "cross" (a, b) -> [d, d], "lmk" [n_lmk, 3, 3]} of a full inverse X: zeros for a constant block, NaN for
        a singular landmark."""
        w, d = self.w, self.d
        kf = np.zeros((w.n_kf, d, d)); lmk = np.zeros((w.n_lmk, 3, 3))
        for k, idx in enumerate(self.kf_idx):
            if idx is not None:
                kf[k] = X[np.ix_(idx, idx)]
        for l, idx in enumerate(self.lmk_idx):
            if idx is not None:
                lmk[l] = X[np.ix_(idx, idx)]
        for l in self.singular:
            lmk[l] = np.nan

        def cross(a, b):
            ia, ib = self.kf_idx[a], self.kf_idx[b]
            return np.zeros((d, d)) if ia is None or ib is None else X[np.ix_(ia, ib)]
        return {"kf": kf, "lmk": lmk, "cross": cross}


def reference_blocks(info):
    return info.blocks_of(np.linalg.inv(info.H))


def rel_diff(got, ref):
    """Relative difference of two blocks: max |got - ref| / max |ref| (0 for two all-zero blocks)."""
    got, ref = np.asarray(got, dtype=np.float64), np.asarray(ref, dtype=np.float64)
    s = np.abs(ref).max()
    e = np.abs(got - ref).max()
    return 0.0 if e == 0.0 else e / s


# ---- the 50-digit yardstick -------------------------------------------------------------------------------------------------------
def mp_inverse_general(H, digits=50):
    """np.array (float64, rounded from 50 digits) of mpmath's inverse of H."""
    import mpmath
    mpmath.mp.dps = digits
    n = H.shape[0]
    X = mpmath.inverse(mpmath.matrix(H.tolist()))
    return np.array([[float(X[i, j]) for j in range(n)] for i in range(n)])


def _mp_spd_inverse(A):
    """Inverse of the symmetric positive definite mpmath matrix A through its Cholesky factor, on plain lists with mpmath.fdot
    (mpmath.inverse spends most of its time in the element access of its dict-based matrix type)."""
    import mpmath
    n = A.rows
    L = [[mpmath.mpf(0)] * n for _ in range(n)]
    for i in range(n):
        for j in range(i + 1):
            s = A[i, j] - mpmath.fdot(L[i][:j], L[j][:j])
            L[i][j] = mpmath.sqrt(s) if i == j else s / L[j][j]
    M = [[mpmath.mpf(0)] * n for _ in range(n)]          # M = L^-1, lower; stored by COLUMN: Mc[j][i] = M[i][j]
    Mc = [[mpmath.mpf(0)] * n for _ in range(n)]
    for j in range(n):
        Mc[j][j] = 1 / L[j][j]
        for i in range(j + 1, n):
            Mc[j][i] = -mpmath.fdot(L[i][j:i], Mc[j][j:i]) / L[i][i]
    X = mpmath.matrix(n, n)
    for i in range(n):
        for j in range(i + 1):
            v = mpmath.fdot(Mc[i][i:], Mc[j][i:])         # sum_k M[k][i] M[k][j], k >= i >= j
            X[i, j] = v; X[j, i] = v
    return X


def mp_blocks(info, digits=50, want_residual=False):
    """Blocks (as Information.blocks_of) of the 50-digit inverse of info.H, the landmarks that couple to no other landmark eliminated
    block-wise. want_residual: also max |H X - I| over the block columns formed, in 50-digit arithmetic."""
    import mpmath
    mpmath.mp.dps = digits
    mpf = mpmath.mpf
    H, n = info.H, info.n
    lcols = [idx for idx in info.lmk_idx if idx is not None]
    is_l = np.zeros(n, dtype=bool)
    for idx in lcols:
        is_l[idx] = True
    elim = []
    for idx in lcols:
        others = is_l.copy(); others[idx] = False
        if not np.any(H[np.ix_(idx, np.flatnonzero(others))]):
            elim.append(idx)
    in_e = np.zeros(n, dtype=bool)
    for idx in elim:
        in_e[idx] = True
    p = np.flatnonzero(~in_e)
    pos = {int(c): i for i, c in enumerate(p)}
    npp = len(p)

    def inv3(M):
        return mpmath.inverse(mpmath.matrix([[mpf(float(v)) for v in row] for row in M]))
    S = mpmath.matrix([[mpf(float(v)) for v in row] for row in H[np.ix_(p, p)]]) if npp else None
    recs = []
    for idx in elim:
        Di = inv3(H[np.ix_(idx, idx)])
        rows = np.flatnonzero(np.any(H[np.ix_(p, idx)] != 0.0, axis=1))         # positions in p that couple to the landmark
        Bm = mpmath.matrix([[mpf(float(H[p[r], c])) for c in idx] for r in rows]) if len(rows) else None
        if Bm is not None:
            BD = Bm * Di
            upd = BD * Bm.T
            for a, ra in enumerate(rows):
                for b, rb in enumerate(rows):
                    S[int(ra), int(rb)] -= upd[a, b]
            recs.append((idx, Di, rows, BD))
        else:
            recs.append((idx, Di, rows, None))
    Spp = _mp_spd_inverse(S) if npp else None
    X = np.zeros((n, n))     # only the blocks asked of it are filled
    for a in range(npp):
        for b in range(npp):
            X[p[a], p[b]] = float(Spp[a, b])
    worst = mpf(0)
    recs_done = []
    for idx, Di, rows, BD in recs:
        recs_done.append(idx)
        blk = Di.copy()
        if BD is not None:
            sub = mpmath.matrix([[Spp[int(ra), int(rb)] for rb in rows] for ra in rows])
            blk = Di + BD.T * sub * BD
        for i in range(3):
            for j in range(3):
                X[idx[i], idx[j]] = float(blk[i, j])
        if want_residual and BD is not None and (len(recs_done) % 16 == 0 or len(rows) >= 100):   # a sample of the landmarks, and every long track
            # the landmark's block column of the inverse: rows p = -Sigma_pp B D^-1, rows l = blk; H X - I on the rows it touches
            colp = -(mpmath.matrix([[Spp[a, int(rb)] for rb in rows] for a in range(npp)]) * BD)     # npp x 3
            Hl = mpmath.matrix([[mpf(float(H[r, c])) for c in idx] for r in idx])
            Bm = mpmath.matrix([[mpf(float(H[p[r], c])) for c in idx] for r in rows])
            res_l = Bm.T * mpmath.matrix([[colp[int(r), j] for j in range(3)] for r in rows]) + Hl * blk - mpmath.eye(3)
            worst = max(worst, max(abs(v) for v in res_l))
    out = info.blocks_of(X)
    if want_residual:
        return out, float(worst)
    return out


def worst_block_difference(a, b, info, pairs=()):
    """Largest rel_diff over every key-frame block, the given cross pairs and every landmark block that is not singular."""
    worst = 0.0
    for k in range(info.w.n_kf):
        worst = max(worst, rel_diff(a["kf"][k], b["kf"][k]))
    for (i, j) in pairs:
        worst = max(worst, rel_diff(a["cross"](i, j), b["cross"](i, j)))
    for l in range(info.w.n_lmk):
        if l not in info.singular:
            worst = max(worst, rel_diff(a["lmk"][l], b["lmk"][l]))
    return worst
