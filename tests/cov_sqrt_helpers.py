"""Test infrastructure of the covariance's square-root assembly (sadvio_amd/csrc/cov_kernels.h: k_cov_assemble_sqrt,
k_cov_schur_sqrt, k_cov_lmk<G, true>): windows with a landmark millimetres from a camera centre, a 50-digit yardstick formed from
the float64 JACOBIAN, and both assemblies of the device restated in NumPy. Nothing here edits cov_helpers.

Why a yardstick of its own: cov_helpers.Information keeps the float64 H = J^T J. With a landmark 0.1 mm from a camera centre that
landmark's share of H_pp is 1e14 beside entries of S of 1e10, and rounding H to float64 has already lost what is tested.
mp_blocks_from_J forms J^T J, the block-wise elimination and the inverse in 50 digits from the float64 J of oracle/twin.py's Problem.

E_REF[case] of the new windows is the larger of
  (i)  float64 Householder QR of the whole J (Sigma = R^-1 R^-T) against the 50-digit blocks, and
  (ii) the spread of the 50-digit blocks when every landmark position and every key-frame translation is nudged one unit in the last
       place, 8 seeded draws (the pattern of tests/conditioning.py::oracle_self_sensitivity): the device is entitled to its own
       last-place rounding of the 0.1 mm depth,
measured by tests/test_cov_sqrt_cpu.py (which asserts that the day's figure lies in (E_REF / 4, E_REF]) and recorded here rounded up.
A device block passes at cov_helpers.TOL_FACTOR = 64 x E_REF; 64 x E_REF <= 1e-6 holds for every window below."""
import dataclasses

import numpy as np

import cov_helpers as ch
from oracle import twin
from sadvio_amd import synthetic

EPS = 2.220446049250313e-16
NEAR_LMK = 79          # the re-placed landmark of window_near
NEAR_KF = (0, 1, 2, 3)  # its observing key-frames (camera 0 of each)

# (i) | (ii) as measured by test_cov_sqrt_cpu.py::test_yardsticks_against_each_other are in that test's docstring
E_REF = {
    "near_1e-3": 3.0e-13,
    "near_1e-4": 3.0e-12,
    "near_1e-3_noisy": 3.2e-13,
    "band_near_1e-4": 3.0e-12,
}
PAIRS = {"near_1e-3": [(0, 1), (1, 0), (0, 4)], "near_1e-4": [(0, 1), (1, 0), (0, 4)], "near_1e-3_noisy": [(0, 1), (1, 0), (0, 4)],
         "band_near_1e-4": [(0, 1), (0, 10), (10, 0)]}
WINDOWS = {"near_1e-3": lambda: window_near(1e-3), "near_1e-4": lambda: window_near(1e-4), "near_1e-3_noisy": lambda: window_near(1e-3, True),
           "band_near_1e-4": lambda: window_band_near(1e-4)}


# ---- windows -------------------------------------------------------------------------------------------------------------------
def _replace_last_landmark(w, p_w, kfs, cam=0):
    """w with its last landmark at p_w (world), observed by camera `cam` of the key-frames kfs with exact projections."""
    l = w.n_lmk - 1
    o0 = int(w.lmk_obs_ptr[l])
    kf, cm, meas = [], [], []
    K = w.cam_K[cam]
    for k in kfs:
        T = synthetic.T12_to_4(w.cam_T_s_f[cam]) @ synthetic.T12_to_4(w.kf_T_f_w[k])
        pc = T[:3, :3] @ p_w + T[:3, 3]
        kf.append(k); cm.append(cam); meas.append([K[0] * pc[0] / pc[2] + K[2], K[1] * pc[1] / pc[2] + K[3]])
    ptr = w.lmk_obs_ptr.copy()
    ptr[l + 1] = o0 + len(kfs)
    lmk_p = w.lmk_p.copy(); lmk_p[l] = p_w
    return dataclasses.replace(
        w, lmk_p=lmk_p, lmk_obs_ptr=ptr.astype(np.int32), obs_kf=np.concatenate([w.obs_kf[:o0], np.array(kf, dtype=np.int32)]).astype(np.int32),
        obs_cam=np.concatenate([w.obs_cam[:o0], np.array(cm, dtype=np.int32)]).astype(np.int32), obs_meas=np.concatenate([w.obs_meas[:o0], np.array(meas)]))


def _near_point(w, k, z, cam=0):
    """(0.3 z, -0.2 z, z) in camera `cam` of key-frame k, in world coordinates."""
    T = synthetic.T12_to_4(w.cam_T_s_f[cam]) @ synthetic.T12_to_4(w.kf_T_f_w[k])
    return np.linalg.solve(T[:3, :3], np.array([0.3 * z, -0.2 * z, z]) - T[:3, 3])


def _views_of(w, p_w, first, n, cam=0, width=752, height=480, border=5.0):
    """The first n key-frames other than `first` whose camera `cam` sees p_w deeper than 0.2 m inside the image."""
    out = []
    K = w.cam_K[cam]
    for k in range(w.n_kf):
        if k == first:
            continue
        T = synthetic.T12_to_4(w.cam_T_s_f[cam]) @ synthetic.T12_to_4(w.kf_T_f_w[k])
        pc = T[:3, :3] @ p_w + T[:3, 3]
        if pc[2] <= 0.2:
            continue
        u, v = K[0] * pc[0] / pc[2] + K[2], K[1] * pc[1] / pc[2] + K[3]
        if border < u < min(width, 2 * K[2]) - border and border < v < min(height, 2 * K[3]) - border:
            out.append(k)
        if len(out) == n:
            break
    assert len(out) == n
    return out


def window_near(z, noisy=False):
    """6 KF x 80 landmarks, pixel factor, 2 m of trajectory, the state at the truth (no perturbation); landmark NEAR_LMK re-placed at
    (0.3 z, -0.2 z, z) in camera 0 of free key-frame 0, seen by that camera and by camera 0 of three older key-frames (0.4 / 0.8 /
    1.2 m behind). Measurements are exact projections, so the solve stays at the constructed state; noisy: 0.3 px of noise on the
    other landmarks' measurements, so that it moves."""
    w = synthetic.make_window(n_kf=6, n_lmk=80, seed=131, length=2.0, pixel_noise=0.3 if noisy else 0.0, rot_perturb_deg=0.0, trans_perturb=0.0,
                              lmk_perturb=0.0)
    p = _near_point(w, 0, z)
    kfs = [0] + _views_of(w, p, 0, 3)
    assert tuple(kfs) == NEAR_KF
    return _replace_last_landmark(w, p, kfs)


def window_band_near(z=1e-4):
    """cov_band_helpers.window_vo12's geometry (same seed; the state at the truth, exact measurements, so that the solve stays) with
    its last landmark re-placed at depth z in camera 0 of the newest key-frame that saw it, observed from that key-frame and the two
    key-frames behind it (inside the band)."""
    w = synthetic.make_window(n_kf=12, n_lmk=200, length=6.0, band=3, seed=3, pixel_noise=0.0, rot_perturb_deg=0.0, trans_perturb=0.0, lmk_perturb=0.0)
    l = w.n_lmk - 1
    k0 = int(w.obs_kf[w.lmk_obs_ptr[l]:w.lmk_obs_ptr[l + 1]].min())
    p = _near_point(w, k0, z)
    kfs = [k0] + _views_of(w, p, k0, 2)
    assert max(kfs) - min(kfs) <= 3
    return _replace_last_landmark(w, p, kfs)


# ---- the Jacobian ----------------------------------------------------------------------------------------------------------------
class Lin:
    """The float64 Jacobian of every residual block of w at `deltas` (oracle/twin.py's Problem, nothing left out) with the index set
    of every key-frame and landmark block, and the rows of every landmark."""

    def __init__(self, w, deltas, huber_a=0.0):
        self.w = w
        P = twin.Problem(twin.Backend("f64"), w, huber_a)
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
        self.J = np.asarray(J, dtype=np.float64)
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
        self.lmk_rows = [None if idx is None else np.flatnonzero(np.any(self.J[:, idx] != 0.0, axis=1)) for idx in self.lmk_idx]
        in_l = np.zeros(self.n, bool)
        for idx in self.lmk_idx:
            if idx is not None:
                in_l[idx] = True
        self.p = np.flatnonzero(~in_l)                       # the reduced system's columns, in the twin's order
        self.pos = {int(c): i for i, c in enumerate(self.p)}
        owner = np.full(self.J.shape[0], -1)
        for l, rows in enumerate(self.lmk_rows):
            if rows is not None:
                assert np.all(owner[rows] == -1)             # no residual block touches two landmarks
                owner[rows] = l
        self.other_rows = np.flatnonzero(owner < 0)
        self.n_obs_of = np.diff(w.lmk_obs_ptr)

    def blocks(self, Spp, lmk, singular):
        """{"kf", "lmk", "cross", "singular"} from the inverse Spp of the reduced system (over self.p) and the landmark blocks."""
        w, d = self.w, self.d
        kf = np.zeros((w.n_kf, d, d))
        sub = [None if idx is None else np.array([self.pos[int(c)] for c in idx]) for idx in self.kf_idx]
        for k, s in enumerate(sub):
            if s is not None:
                kf[k] = Spp[np.ix_(s, s)]

        def cross(a, b):
            return np.zeros((d, d)) if sub[a] is None or sub[b] is None else Spp[np.ix_(sub[a], sub[b])]
        return {"kf": kf, "lmk": lmk, "cross": cross, "singular": sorted(singular)}


def worst(a, b, lin, pairs=()):
    """Largest cov_helpers.rel_diff over every key-frame block, the given pairs and every landmark block that is not singular in b."""
    m = 0.0
    for k in range(lin.w.n_kf):
        m = max(m, ch.rel_diff(a["kf"][k], b["kf"][k]))
    for (i, j) in pairs:
        m = max(m, ch.rel_diff(a["cross"](i, j), b["cross"](i, j)))
    for l in range(lin.w.n_lmk):
        if l not in b["singular"]:
            m = max(m, ch.rel_diff(a["lmk"][l], b["lmk"][l]))
    return m


# ---- the 50-digit yardstick --------------------------------------------------------------------------------------------------------
def mp_blocks_from_J(w, deltas, huber=0.0, digits=50, lin=None):
    """Blocks of the inverse of J^T J with J^T J, the block-wise elimination of the landmarks and the inverse of the reduced system
    all in `digits`-digit arithmetic, from the float64 J. A free landmark with fewer than two observations is left out with its
    rows and reported NaN (cov_helpers.singular_landmarks)."""
    import mpmath
    mpmath.mp.dps = digits
    mpf = mpmath.mpf
    lin = lin or Lin(w, deltas, huber)
    J, p, npp = lin.J, lin.p, len(lin.p)
    singular = set(ch.singular_landmarks(w))

    def gram(rows, ca, cb):
        A = mpmath.matrix([[mpf(float(J[r, c])) for c in ca] for r in rows])
        B = A if cb is ca else mpmath.matrix([[mpf(float(J[r, c])) for c in cb] for r in rows])
        return A.T * B
    S = mpmath.matrix(npp, npp)

    def add(cols, M, sign=1):
        for i, ci in enumerate(cols):
            for j, cj in enumerate(cols):
                S[lin.pos[int(ci)], lin.pos[int(cj)]] += sign * M[i, j]
    for r in lin.other_rows:
        cols = [c for c in np.flatnonzero(J[r] != 0.0)]
        add(cols, gram([r], cols, cols))
    recs = {}
    for l, idx in enumerate(lin.lmk_idx):
        if idx is None or l in singular:
            continue
        rows = lin.lmk_rows[l]
        cols = [c for c in p if np.any(J[rows, c] != 0.0)]
        Di = mpmath.inverse(gram(rows, idx, idx))
        for r in rows:                                       # H_pp row by row: a row touches one key-frame's columns
            cr = [c for c in cols if J[r, c] != 0.0]
            add(cr, gram([r], cr, cr))
        if cols:
            B = gram(rows, cols, idx)                        # H_pl
            BD = B * Di
            add(cols, BD * B.T, -1)
            recs[l] = (Di, cols, BD)
        else:
            recs[l] = (Di, cols, None)
    Spp_mp = ch._mp_spd_inverse(S) if npp else None
    Spp = np.array([[float(Spp_mp[i, j]) for j in range(npp)] for i in range(npp)]) if npp else np.zeros((0, 0))
    lmk = np.zeros((w.n_lmk, 3, 3))
    for l in singular:
        lmk[l] = np.nan
    for l, (Di, cols, BD) in recs.items():
        blk = Di
        if BD is not None:
            s = [lin.pos[int(c)] for c in cols]
            sub = mpmath.matrix([[Spp_mp[a, b] for b in s] for a in s])
            blk = Di + BD.T * sub * BD
        lmk[l] = [[float(blk[i, j]) for j in range(3)] for i in range(3)]
    return lin.blocks(Spp, lmk, singular)


def qr_blocks(lin):
    """Yardstick (i): float64 Householder QR of the whole J (the rows and columns of the landmarks with fewer than two observations
    left out), Sigma = R^-1 R^-T."""
    w = lin.w
    singular = set(ch.singular_landmarks(w))
    keep_r = np.ones(lin.J.shape[0], bool); keep_c = np.ones(lin.n, bool)
    for l in singular:
        keep_r[lin.lmk_rows[l]] = False; keep_c[lin.lmk_idx[l]] = False
    cols = np.flatnonzero(keep_c)
    R = np.linalg.qr(lin.J[np.ix_(np.flatnonzero(keep_r), cols)], mode="r")
    Ri = np.linalg.solve(R, np.eye(len(cols)))
    X = np.zeros((lin.n, lin.n))
    X[np.ix_(cols, cols)] = Ri @ Ri.T
    lmk = np.zeros((w.n_lmk, 3, 3))
    for l, idx in enumerate(lin.lmk_idx):
        if idx is not None:
            lmk[l] = np.nan if l in singular else X[np.ix_(idx, idx)]
    return lin.blocks(X[np.ix_(lin.p, lin.p)], lmk, singular)


def nudged(w, seed):
    """w with every landmark coordinate and every key-frame translation moved one unit in the last place, up or down."""
    rng = np.random.default_rng(seed)

    def nudge(a):
        a = np.asarray(a, dtype=np.float64)
        return np.where(rng.random(a.shape) < 0.5, np.nextafter(a, np.inf), np.nextafter(a, -np.inf))
    T = w.kf_T_f_w.copy().reshape(w.n_kf, 3, 4)
    T[:, :, 3] = nudge(T[:, :, 3])
    return dataclasses.replace(w, lmk_p=nudge(w.lmk_p), kf_T_f_w=T.reshape(w.kf_T_f_w.shape))


# ---- the pivot tests of S (marg_kernels.h: k_wfac_diag; cov_batch_kernels.h; cov_band_kernels.h) ----------------------------------
def pivots_pass(S):
    """Unpivoted Cholesky of S with the device's three tests of every pivot: finite, above 1e-12 / N_p, and not below
    1024 N_p eps of its diagonal entry of S."""
    n = S.shape[0]
    L = np.zeros((n, n))
    for j in range(n):
        d = S[j, j] - L[j, :j] @ L[j, :j]
        if not np.isfinite(d) or not d > 1e-12 / max(n, 1) or d < 1024.0 * n * EPS * S[j, j]:
            return False
        L[j, j] = np.sqrt(d)
        L[j + 1:, j] = (S[j + 1:, j] - L[j + 1:, :j] @ L[j, :j]) / L[j, j]
    return True


def _finish(lin, S, per_lmk, singular, lmk_block):
    """Sigma_pp = S^-1 through the Cholesky factor (as the device: triangular inverse, Z^T Z) and the landmark blocks."""
    w = lin.w
    lmk = np.zeros((w.n_lmk, 3, 3))
    for l in singular:
        lmk[l] = np.nan
    S = 0.5 * (S + S.T)
    if len(lin.p) and not pivots_pass(S):
        return {"usable": False, "singular": sorted(singular)}
    if len(lin.p):
        Z = np.linalg.inv(np.linalg.cholesky(S))
        Spp = Z.T @ Z
    else:
        Spp = np.zeros((0, 0))
    for l, rec in per_lmk.items():
        lmk[l] = lmk_block(rec, Spp)
    out = lin.blocks(Spp, lmk, singular)
    out["usable"] = True
    return out


def _sym3_inverse(a):
    """cov_sym3_inverse: the 3 x 3 inverse through the Cholesky factor, None when a pivot is not above 64 ulps of its diagonal entry."""
    tol = 64.0 * EPS
    if not a[0, 0] > 0.0:
        return None
    l00 = np.sqrt(a[0, 0]); l10 = a[0, 1] / l00; l20 = a[0, 2] / l00
    d1 = a[1, 1] - l10 * l10
    if not d1 > tol * a[1, 1]:
        return None
    l11 = np.sqrt(d1); l21 = (a[1, 2] - l20 * l10) / l11
    d2 = a[2, 2] - l20 * l20 - l21 * l21
    if not d2 > tol * a[2, 2]:
        return None
    L = np.array([[l00, 0, 0], [l10, l11, 0], [l20, l21, np.sqrt(d2)]])
    M = np.linalg.inv(L)
    return M.T @ M


def plain_form_blocks(lin):
    """k_cov_assemble / k_cov_schur / k_cov_lmk restated: H_ll, H_ll^-1, W = H_ll^-1 H_lp, S = H_pp - sum W^T H_ll W,
    Sigma_ll = H_ll^-1 + W Sigma_pp W^T."""
    J, p = lin.J, lin.p
    S = J[np.ix_(lin.other_rows, p)].T @ J[np.ix_(lin.other_rows, p)]
    singular, per = set(), {}
    for l, idx in enumerate(lin.lmk_idx):
        if idx is None:
            continue
        rows = lin.lmk_rows[l]
        Jl, Jp = J[np.ix_(rows, idx)], J[np.ix_(rows, p)]
        H = Jl.T @ Jl
        Hi = _sym3_inverse(H) if lin.n_obs_of[l] >= 2 else None
        if Hi is None:
            singular.add(l)
            continue
        Wl = Hi @ (Jl.T @ Jp)
        S += Jp.T @ Jp
        S -= Wl.T @ (H @ Wl)
        per[l] = (Hi, Wl)
    return _finish(lin, S, per, singular, lambda rec, Spp: rec[0] + rec[1] @ Spp @ rec[1].T)


def gram_schmidt_2(Jl):
    """k_cov_assemble_sqrt's factorisation: column after column, two orthogonalisation passes against the columns before it.
    (Q1, R), or None when r_jj^2 <= 64 eps |column j|^2."""
    Q = np.array(Jl, dtype=np.float64)
    R = np.zeros((3, 3))
    cn = (Jl * Jl).sum(axis=0)
    for j in range(3):
        for _ in range(2):
            for k in range(j):
                s = Q[:, k] @ Q[:, j]
                Q[:, j] -= s * Q[:, k]
                R[k, j] += s
        nn = Q[:, j] @ Q[:, j]
        if not nn > 64.0 * EPS * cn[j]:
            return None
        R[j, j] = np.sqrt(nn)
        Q[:, j] /= R[j, j]
    return Q, R


def sqrt_form_blocks(lin, drop_q_row_of=None, drop_from_list=None):
    """k_cov_assemble_sqrt / k_cov_schur_sqrt / k_cov_lmk<G, true> restated: J_l = Q1 R, C = Q1^T J_p, S = sum_r A[r]^T A[r] with
    A = J_p - Q1 C, Sigma_ll = R^-1 (I + C Sigma_pp C^T) R^-T.
    Planted defects: drop_q_row_of = l: the first row of landmark l's Q1 is left out of its projection; drop_from_list = (l, k):
    landmark l is missing from key-frame k's list, so the pairs (k, .) with k the larger free index never see it."""
    J, p = lin.J, lin.p
    S = J[np.ix_(lin.other_rows, p)].T @ J[np.ix_(lin.other_rows, p)]
    singular, per = set(), {}
    for l, idx in enumerate(lin.lmk_idx):
        if idx is None:
            continue
        rows = lin.lmk_rows[l]
        Jl, Jp = J[np.ix_(rows, idx)], J[np.ix_(rows, p)]
        qr = gram_schmidt_2(Jl) if lin.n_obs_of[l] >= 2 else None
        if qr is None:
            singular.add(l)
            continue
        Q, R = qr
        Cl = Q.T @ Jp
        Qp = Q.copy()
        if drop_q_row_of == l:
            Qp[0] = 0.0
        A = Jp - Qp @ Cl
        G = A.T @ A
        if drop_from_list is not None and drop_from_list[0] == l:
            s = np.array([lin.pos[int(c)] for c in lin.kf_idx[drop_from_list[1]]])
            lower = np.arange(len(p)) <= s.max()               # pairs (k, b), b <= k in free index: walked from k's list
            G[np.ix_(s, np.flatnonzero(lower))] = 0.0
            G[np.ix_(np.flatnonzero(lower), s)] = 0.0
        S += G
        per[l] = (R, Cl)

    def lmk_block(rec, Spp):
        R, Cl = rec
        U = np.linalg.inv(R)
        return U @ (np.eye(3) + Cl @ Spp @ Cl.T) @ U.T
    return _finish(lin, S, per, singular, lmk_block)


# ---- the device against a yardstick ------------------------------------------------------------------------------------------------
def device_worst(c, ref, lin, pairs=(), want_kf=True):
    """{"kf", "pair", "lmk"}: the largest rel_diff of a Backend.covariance result (all key-frames, `pairs`, all landmarks) from ref;
    singular landmarks must be NaN on both sides."""
    m = {"kf": 0.0, "pair": 0.0, "lmk": 0.0}
    if want_kf:
        for k in range(lin.w.n_kf):
            m["kf"] = max(m["kf"], ch.rel_diff(c["kf"][k], ref["kf"][k]))
    for i, (a, b) in enumerate(pairs):
        m["pair"] = max(m["pair"], ch.rel_diff(c["pair"][i], ref["cross"](a, b)))
    for l in range(lin.w.n_lmk):
        if l in ref["singular"]:
            assert np.isnan(c["lmk"][l]).all(), l
        else:
            assert np.isfinite(c["lmk"][l]).all(), l
            m["lmk"] = max(m["lmk"], ch.rel_diff(c["lmk"][l], ref["lmk"][l]))
    return m
