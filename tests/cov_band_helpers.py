"""Test infrastructure of the covariance's band route (sadvio_amd/csrc/cov_band_kernels.h): the windows of
tests/test_gpu_cov_band.py, their float64 yardsticks, the bandwidth rule and the selected inversion restated in NumPy, the same
recursion in 50 digits, and a block-sparse Schur reference for the window that is too large for cov_helpers.Information's dense
Jacobian. Nothing here edits cov_helpers; the bar is its rule: a device block passes at TOL_FACTOR x E_REF of its window.

E_REF[case] = the largest relative block difference between the float64 inverse and the 50-digit one on that window at the oracle's
solution (every key-frame block, the case's pairs, every landmark block; for "at_size" the blocks the GPU test asks for, the float64
side being the Schur reference below and the 50-digit side band_blocks_50_digits). Measured by tests/test_cov_band_cpu.py, which
asserts that the day's figure lies in (E_REF / 4, E_REF]; recorded here rounded up."""
import dataclasses
import functools

import numpy as np

import cov_helpers as ch
from sadvio_amd import capi, synthetic

E_REF = {
    "vo12": 5.5e-12,
    "vo12_angular": 5.0e-12,
    "vo40": 9.5e-12,
    "vio8": 9.5e-13,
    "relpose": 2.3e-12,
    "huber": 1.6e-12,
    "at_size": 8.0e-8,
}


# ---- windows --------------------------------------------------------------------------------------------------------------------
def window_vo12(factor=capi.FACTOR_PIXEL):
    """12 key-frames, 11 free: N_p = 66, bw = 30 — the band route's LDS image (36 columns) slides over several block columns."""
    return synthetic.make_window(n_kf=12, n_lmk=200, length=6.0, band=3, seed=3, factor=factor)


def window_vo40():
    """40 key-frames: N_p = 234, bw = 54. The solve of this window is out of LDS."""
    return synthetic.make_window(n_kf=40, n_lmk=600, length=20.0, band=5, seed=11)


def window_vio8():
    """tests/test_gpu_large.py::test_vio_window_out_of_lds at reduced size: 8 key-frames with IMU states and seven IMU pairs,
    15 x 15 blocks, block columns of 5."""
    from vio_helpers import make_vio_window
    return make_vio_window(n_kf=8, n_lmk=160, seed=17, length=4.0, band=1)


RELPOSE_KF = (1, 8)   # key-frames of the relative-pose factor: further apart than any landmark of window_vo12 couples


def window_relpose():
    from test_oracle_relative import relative_prior
    w = window_vo12()
    a, b = RELPOSE_KF
    rng = np.random.default_rng(5)
    W = np.diag(rng.uniform(20, 60, 6)) + rng.standard_normal((6, 6))
    w.sparse_priors = list(getattr(w, "sparse_priors", None) or [])
    w.sparse_priors.append(dict(type=capi.SPARSE_RELATIVE_POSE, kf=a, kf_b=b, T_prior=relative_prior(w.kf_T_f_w[a], w.kf_T_f_w[b]), sqrt_inf=W))
    return w


def window_huber():
    """window_vo12 with three gross outliers (solved under HuberLoss(sqrt(1.345)))."""
    w = window_vo12()
    meas = w.obs_meas.copy()
    for o, d in ((5, (60.0, -45.0)), (50, (-80.0, 30.0)), (100, (40.0, 70.0))):
        meas[o] += d
    w.obs_meas = meas
    return w


AT_SIZE_N_KF = 345


@functools.lru_cache(maxsize=1)
def window_at_size():
    """345 key-frames, 344 free: N_p = 2 064, past the dense route's 2 047 columns. About 9 landmarks seeded per key-frame, half a
    metre between key-frames as in the other long windows. The seed is chosen on the CPU side: at seed 3 the largest entry of H_pp
    at the oracle's solution is 8.9e11 and S, formed as k_cov_schur forms it (H_pp - sum W^T H_ll W with W = H_ll^-1 H_lp), differs
    from the Schur complement by 4e-4 absolute. At seeds 1, 2, 6 and 29 the solve of these thinly observed windows leaves one
    landmark within centimetres of a camera centre, H_pp reaches 1e14 .. 1e18 beside entries of S of 1e10, and that form cancels to
    a matrix float64 no longer finds positive definite (measured on the CPU: smallest eigenvalue -6e3 at seed 29, -2e5 at seed 1):
    the covariance then returns SADVIO_E_NOT_USABLE on either route, the dense one included (seen at 300 key-frames, N_p = 1 794).
    That is a limit of the assembly, which the band route leaves as it is."""
    return synthetic.make_window(n_kf=AT_SIZE_N_KF, n_lmk=9 * AT_SIZE_N_KF, length=172.5, band=3, seed=3)


WINDOWS = {   # case -> (builder, huber_a)
    "vo12": (window_vo12, 0.0),
    "vo12_angular": (lambda: window_vo12(capi.FACTOR_ANGULAR), 0.0),
    "vo40": (window_vo40, 0.0),
    "vio8": (window_vio8, 0.0),
    "relpose": (window_relpose, 0.0),
    "huber": (window_huber, ch.HUBER_A),
}


# ---- the bandwidth rule (solve_driver.h: window_bandwidth) -----------------------------------------------------------------------
def free_index(w):
    """Free key-frame index per key-frame of w (-1: constant)."""
    const = np.zeros(w.n_kf, bool) if w.kf_const is None else np.asarray(w.kf_const).astype(bool)
    return np.where(const, -1, np.cumsum(~const) - 1)


def bandwidth(w):
    """(hb, bw, dpf): the largest free-key-frame distance a landmark, an IMU pair or a relative-pose factor couples; (hb + 1) dpf."""
    f = free_index(w)
    dpf = 15 if w.has_imu else 6
    hb = 0
    for l in range(w.n_lmk):
        k = f[w.obs_kf[w.lmk_obs_ptr[l]:w.lmk_obs_ptr[l + 1]]]
        k = k[k >= 0]
        if len(k):
            hb = max(hb, int(k.max() - k.min()))
    for fac in (getattr(w, "imu_factors", None) or []):
        a, b = f[fac["kf_i"]], f[fac["kf_j"]]
        if a >= 0 and b >= 0:
            hb = max(hb, abs(int(a - b)))
    for fac in (getattr(w, "sparse_priors", None) or []):
        if fac["type"] == capi.SPARSE_RELATIVE_POSE:
            a, b = f[fac["kf"]], f[fac["kf_b"]]
            if a >= 0 and b >= 0:
                hb = max(hb, abs(int(a - b)))
    n_free = int((f >= 0).sum())
    return hb, min(n_free * dpf, (hb + 1) * dpf), dpf


def block_column(dpf):
    return 6 if dpf == 6 else 5


def in_band_pairs(w, hb):
    f = free_index(w)
    free = [k for k in range(w.n_kf) if f[k] >= 0]
    return [(a, b) for a in free for b in free if a != b and abs(f[a] - f[b]) <= hb]


# ---- S and the selected inversion in NumPy ---------------------------------------------------------------------------------------
def schur(info):
    """(S, cols): the reduced system of info.H over the free key-frame states in the device's order (free key-frame after free
    key-frame, pose6 | v3 | ba3 | bg3), the landmarks eliminated; cols[k] = first column of key-frame k (-1: constant)."""
    p = np.concatenate([idx for idx in info.kf_idx if idx is not None])
    is_p = np.zeros(info.n, bool); is_p[p] = True
    l = np.flatnonzero(~is_p)
    H = info.H
    S = H[np.ix_(p, p)]
    if len(l):
        S = S - H[np.ix_(p, l)] @ np.linalg.solve(H[np.ix_(l, l)], H[np.ix_(l, p)])
    cols, c = [], 0
    for idx in info.kf_idx:
        cols.append(-1 if idx is None else c)
        c += 0 if idx is None else info.d
    return 0.5 * (S + S.T), np.array(cols)


def band_selected_inverse(S, bw, nb, drop_last_block_row=False):
    """The entries of S^-1 at |i - j| < bw + nb - 1 of a matrix with no non-zero at |i - j| >= bw, NaN elsewhere: S = L L^T, then
    block column after block column (nb wide) from the last to the first, J the rows below it inside the band:
        Sigma_Jj = -Sigma_JJ L_Jj L_jj^-1        Sigma_jj = (L_jj^-T - Sigma_Jj^T L_Jj) L_jj^-1
    (what k_cov_band_sel computes). drop_last_block_row: the planted defect of the CPU test, J one block row short."""
    n = S.shape[0]
    assert n % nb == 0
    L = np.linalg.cholesky(S)
    X = np.full((n, n), np.nan)
    for c0 in range(n - nb, -1, -nb):
        r0, r1 = c0 + nb, min(n, c0 + nb + bw - 1)
        if drop_last_block_row:
            r1 = max(r0, r1 - nb)
        Ljj = L[c0:r0, c0:r0]
        Li = np.linalg.inv(Ljj)
        if r1 > r0:
            LJ = L[r0:r1, c0:r0]
            XJ = -X[r0:r1, r0:r1] @ LJ @ Li
            X[r0:r1, c0:r0] = XJ
            X[c0:r0, r0:r1] = XJ.T
            D = (Li.T - XJ.T @ LJ) @ Li
        else:
            D = Li.T @ Li
        X[c0:r0, c0:r0] = 0.5 * (D + D.T)
    return X


def blocks_of_reduced(info, X, cols, pairs=()):
    """{"kf" [n_kf, d, d], "pair" [len(pairs), d, d]} of a reduced-system inverse X (zeros for a constant key-frame)."""
    d = info.d
    kf = np.zeros((info.w.n_kf, d, d))
    for k, c in enumerate(cols):
        if c >= 0:
            kf[k] = X[c:c + d, c:c + d]
    pr = np.zeros((len(pairs), d, d))
    for i, (a, b) in enumerate(pairs):
        if cols[a] >= 0 and cols[b] >= 0:
            pr[i] = X[cols[a]:cols[a] + d, cols[b]:cols[b] + d]
    return {"kf": kf, "pair": pr}


# ---- the same recursion in 50 digits ---------------------------------------------------------------------------------------------
def _mp_band_cholesky(S, bw):
    """L (list of rows, mpmath numbers; entries at |i - j| >= bw are None) of the mpmath-valued band matrix S (callable (i, j))."""
    import mpmath
    n = S.n
    L = [dict() for _ in range(n)]
    for i in range(n):
        for j in range(max(0, i - bw + 1), i + 1):
            lo = max(0, i - bw + 1)
            s = S(i, j) - mpmath.fdot((L[i][k] for k in range(lo, j)), (L[j].get(k, 0) for k in range(lo, j)))
            L[i][j] = mpmath.sqrt(s) if i == j else s / L[j][j]
    return L


class _MpBand:
    def __init__(self, n, bw):
        import mpmath
        self.n, self.bw, self.a, self.zero = n, bw, dict(), mpmath.mpf(0)

    def __call__(self, i, j):
        return self.a.get((max(i, j), min(i, j)), self.zero)

    def add(self, i, j, v):
        if i >= j:
            assert i - j < self.bw
            self.a[(i, j)] = self.a.get((i, j), self.zero) + v


def mp_band_inverse(S, bw, columns=(), digits=50):
    """(band, cols): band[(i, j)] = (S^-1)[i][j] for |i - j| < bw, i >= j, by the scalar Takahashi recursion on the 50-digit band
    Cholesky factor of the _MpBand S; cols[c] = the whole column c of S^-1 (list) by band substitution, for c in `columns`."""
    import mpmath
    mpmath.mp.dps = digits
    n = S.n
    L = _mp_band_cholesky(S, bw)
    X = dict()

    def x(i, j):
        return X[(i, j)] if i >= j else X[(j, i)]
    for j in range(n - 1, -1, -1):
        hi = min(n, j + bw)
        ljj = L[j][j]
        col = [L[k][j] / ljj for k in range(j + 1, hi)]
        for i in range(hi - 1, j, -1):      # Sigma_ij = -sum_k Sigma_ik L_kj / L_jj over the rows k below j
            X[(i, j)] = -mpmath.fdot((x(i, k) for k in range(j + 1, hi)), col)
        X[(j, j)] = 1 / (ljj * ljj) - mpmath.fdot((X[(k, j)] for k in range(j + 1, hi)), col)
    cols = {}
    for c in columns:
        y = [mpmath.mpf(0)] * n
        for i in range(c, n):
            lo = max(c, i - bw + 1)
            y[i] = ((1 if i == c else 0) - mpmath.fdot((L[i][k] for k in range(lo, i)), y[lo:i])) / L[i][i]
        z = [mpmath.mpf(0)] * n
        for i in range(n - 1, -1, -1):
            hi = min(n, i + bw)
            z[i] = (y[i] - mpmath.fdot((L[k][i] for k in range(i + 1, hi)), z[i + 1:hi])) / L[i][i]
        cols[c] = z
    return X, cols


# ---- block-sparse Schur reference ------------------------------------------------------------------------------------------------
class SchurBlocks:
    """The reduced system of a VO window at a state as blocks, for a window whose full Jacobian does not fit: the landmarks go
    through cov_helpers.Information in chunks (a sub-window with every key-frame and the chunk's landmarks; the pose priors ride the
    first chunk only), so every float64 entry of H is the one Information forms. Holds H_pp (dense N_p x N_p, banded), and per
    landmark its H_ll (3 x 3), the reduced columns it couples to and H_pl on them."""

    def __init__(self, w, deltas, huber_a=0.0, chunk=150):
        assert not w.has_imu
        f = free_index(w)
        self.w, self.d = w, 6
        self.cols = np.where(f >= 0, 6 * f, -1)
        self.n = 6 * int((f >= 0).sum())
        self.Hpp = np.zeros((self.n, self.n))
        self.Hll, self.rows, self.Hpl = [None] * w.n_lmk, [None] * w.n_lmk, [None] * w.n_lmk
        self.singular = ch.singular_landmarks(w)
        for c0 in range(0, w.n_lmk, chunk):
            ls = list(range(c0, min(w.n_lmk, c0 + chunk)))
            sub = ch._assemble(w, [(w, l, None) for l in ls])
            if c0 > 0:
                sub.pose_priors = []
            info = ch.Information(sub, {"pose": deltas["pose"], "lmk": deltas["lmk"][ls]}, huber_a)
            p = np.concatenate([idx for idx in info.kf_idx if idx is not None])
            assert len(p) == self.n
            self.Hpp += info.H[np.ix_(p, p)]
            for q, l in enumerate(ls):
                idx = info.lmk_idx[q]
                if idx is None or q in info.singular:
                    continue
                B = info.H[np.ix_(p, idx)]
                rows = np.flatnonzero(np.any(B != 0.0, axis=1))
                self.Hll[l], self.rows[l], self.Hpl[l] = info.H[np.ix_(idx, idx)].copy(), rows, B[rows].copy()

    def S(self):
        S = self.Hpp.copy()
        for l in range(self.w.n_lmk):
            if self.Hll[l] is not None:
                B = self.Hpl[l]
                S[np.ix_(self.rows[l], self.rows[l])] -= B @ np.linalg.solve(self.Hll[l], B.T)
        return 0.5 * (S + S.T)

    def blocks(self, kf, pairs, lmk):
        """float64: {"kf", "pair", "lmk"} for the key-frames, pairs and landmarks named, from np.linalg.inv of S."""
        X = np.linalg.inv(self.S())
        out = {"kf": np.zeros((len(kf), 6, 6)), "pair": np.zeros((len(pairs), 6, 6)), "lmk": np.zeros((len(lmk), 3, 3))}
        c = self.cols
        for i, k in enumerate(kf):
            if c[k] >= 0:
                out["kf"][i] = X[c[k]:c[k] + 6, c[k]:c[k] + 6]
        for i, (a, b) in enumerate(pairs):
            if c[a] >= 0 and c[b] >= 0:
                out["pair"][i] = X[c[a]:c[a] + 6, c[b]:c[b] + 6]
        for i, l in enumerate(lmk):
            if self.Hll[l] is None:
                out["lmk"][i] = np.nan
                continue
            Di = np.linalg.inv(self.Hll[l])
            Wl = self.Hpl[l] @ Di
            out["lmk"][i] = Di + Wl.T @ X[np.ix_(self.rows[l], self.rows[l])] @ Wl
        return out

    def blocks_50_digits(self, bw, kf, pairs, lmk, digits=50):
        """The same blocks in 50-digit arithmetic from the same float64 entries: landmark 3 x 3 blocks, band Cholesky and the
        Takahashi recursion in mpmath; a pair outside the band by band substitution."""
        import mpmath
        mpmath.mp.dps = digits
        mpf = mpmath.mpf
        S = _MpBand(self.n, bw)
        nz = np.argwhere(np.tril(self.Hpp) != 0.0)
        for i, j in nz:
            S.add(int(i), int(j), mpf(float(self.Hpp[i, j])))
        recs = {}
        for l in range(self.w.n_lmk):
            if self.Hll[l] is None:
                continue
            Di = mpmath.inverse(mpmath.matrix([[mpf(float(v)) for v in row] for row in self.Hll[l]]))
            Bm = mpmath.matrix([[mpf(float(v)) for v in row] for row in self.Hpl[l]])
            BD = Bm * Di
            upd = BD * Bm.T
            rows = self.rows[l]
            for a, ra in enumerate(rows):
                for b, rb in enumerate(rows):
                    S.add(int(ra), int(rb), -upd[a, b])
            if l in lmk:
                recs[l] = (Di, BD)
        c = self.cols
        need = sorted({int(c[min(a, b, key=lambda k: c[k])]) + q for (a, b) in pairs if c[a] >= 0 and c[b] >= 0 and abs(c[a] - c[b]) >= bw
                       for q in range(6)})
        X, colsx = mp_band_inverse(S, bw, need, digits)

        def x(i, j):
            if abs(i - j) < bw:
                return X[(max(i, j), min(i, j))]
            return colsx[min(i, j)][max(i, j)]
        out = {"kf": np.zeros((len(kf), 6, 6)), "pair": np.zeros((len(pairs), 6, 6)), "lmk": np.zeros((len(lmk), 3, 3))}
        for i, k in enumerate(kf):
            if c[k] >= 0:
                out["kf"][i] = [[float(x(c[k] + r, c[k] + s)) for s in range(6)] for r in range(6)]
        for i, (a, b) in enumerate(pairs):
            if c[a] >= 0 and c[b] >= 0:
                out["pair"][i] = [[float(x(c[a] + r, c[b] + s)) for s in range(6)] for r in range(6)]
        for i, l in enumerate(lmk):
            if l not in recs:
                out["lmk"][i] = np.nan
                continue
            Di, BD = recs[l]
            rows = [int(r) for r in self.rows[l]]
            sub = mpmath.matrix([[x(ra, rb) for rb in rows] for ra in rows])
            blk = Di + BD.T * sub * BD
            out["lmk"][i] = [[float(blk[r, s]) for s in range(3)] for r in range(3)]
        return out


def at_size_request(w, hb):
    """What the at-size GPU test asks for: the first, middle and last free key-frame, one pair inside the band and one outside
    (both orders), 20 landmarks spread over the window."""
    f = free_index(w)
    free = [k for k in range(w.n_kf) if f[k] >= 0]
    kf = [free[0], free[len(free) // 2], free[-1]]
    mid = free[len(free) // 2]
    pairs = [(mid, free[len(free) // 2 + hb]), (free[3], free[-5]), (free[-5], free[3])]
    sing = set(ch.singular_landmarks(w))
    lmk = [l for l in range(7, w.n_lmk, w.n_lmk // 20) if l not in sing][:20]
    return kf, pairs, lmk


def worst(got, ref):
    """Largest cov_helpers.rel_diff over the blocks of two {"kf", "pair", "lmk"} dicts (NaN blocks must match as NaN)."""
    m = 0.0
    for key in ("kf", "pair", "lmk"):
        for a, b in zip(got.get(key, ()), ref.get(key, ())):
            if np.isnan(b).all():
                assert np.isnan(a).all()
                continue
            m = max(m, ch.rel_diff(a, b))
    return m
