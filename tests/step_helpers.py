"""The 50-digit first LM step (test infrastructure): the yardstick of tests/test_gpu_first_step.py and tests/test_step_reference_cpu.py.

mp_first_step(w, opts) takes the oracle's un-reduced normal equations at x = 0 (H_full, g_full of oracle_first_step: float64, taken as
exact inputs; ordering [free key-frame blocks | kept landmarks | eliminated landmarks]) and solves Ceres' LM system in mpmath:

    s_i   = 1 / (1 + sqrt(H_ii))                                  the Jacobi scale of iteration 0 (s_i = 1 if switched off)
    D2_i  = clamp(s_i^2 H_ii, min_lm_diagonal, max_lm_diagonal) / radius_0 / s_i^2     Ceres' LM diagonal, back in the unscaled variables
    (H + D2) y = g,   step = -y,   model cost change = y.g - y.H.y / 2 = (y.g + y.D2.y) / 2

which is oracle_first_step's compute_step (oracle/solver.c) and twin.lm_solve's first iteration (the scaled system
(S H S + D2s) ys = S g with y = S ys is the same system multiplied through by S^-1). The 3 x 3 blocks of the eliminated landmarks are
eliminated in mpmath (exact algebra), the reduced part is factored by an ENVELOPE Cholesky on plain lists with mpmath.fdot: row i
starts at its first non-zero column, so a banded system costs N bw^2 and a dense one N^3 / 6. The cost after the step is the twin's
(oracle/twin.py) evaluation of every residual block at the 50-digit candidate, in 50-digit arithmetic.

E_REF[case] = (pose part, landmark part) of step_error(oracle's float64 first step, 50-digit step), measured by
tests/test_step_reference_cpu.py and recorded here rounded up; a device step passes at TOL_FACTOR x max(E_REF, FLOOR).

CASES lists every window of the GPU test: OLD_CASES, one per size and route of the reduced solve, and TILE_CASES, one per variant of
the tile kernels (each with the switches that reach it, the kernels that must run and the tiles the planner must give it:
tests/test_tile_plan_cpu.py). A case whose reference costs more than a few seconds of Python reads it from
tests/golden/first_step_ref.npz (tests/golden/make_golden_first_step.py writes it).

tile_host_model_step is a float64 host model of the tile kernels with planted defects (tests/test_step_reference_cpu.py proves with it
that the bar sees them). The last section holds the SECOND step (tests/test_gpu_second_step.py) to the twin's own 50-digit LM loop."""
import ctypes as C
import dataclasses
import os

import numpy as np

from sadvio_amd import capi, synthetic

TOL_FACTOR = 64.0
FLOOR = 8.0 * 2.0 ** -53          # a few roundings on the largest component: e_ref of a well-conditioned case can fall below it
MAX_LDS_NP = 174                  # ba_types.h
WD = 96                           # dense_chol.h: column count of a wide panel
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "first_step_ref.npz")


# ---- layout of the reduced vector (ctx_init of oracle/solver.c; the device's N_p) -------------------------------------------------
def layout(w):
    """dpf, kf_off [n_kf] (-1 constant), lmk_red [n_lmk] (column of a kept landmark in the reduced vector, else -1), lmk_col [n_lmk]
    (column of an eliminated landmark in the un-reduced vector, else -1), Nr, N."""
    dpf = 15 if int(getattr(w, "has_imu", 0)) else 6
    kc = np.asarray(w.kf_const).astype(bool)
    lc = np.zeros(w.n_lmk, bool) if getattr(w, "lmk_const", None) is None else np.asarray(w.lmk_const).astype(bool)
    kf_off = np.full(w.n_kf, -1)
    off = 0
    for k in range(w.n_kf):
        if not kc[k]:
            kf_off[k] = off; off += dpf
    lmk_red = np.full(w.n_lmk, -1)
    dp = getattr(w, "dense_prior", None)
    if dp is not None:
        for li, col in zip(dp["lmk_index"], dp["lmk_col"]):
            if col >= 0 and not lc[int(li)]:
                lmk_red[int(li)] = off; off += 3
    assert not getattr(w, "sparse_priors", None) and getattr(w, "lines", None) is None
    Nr = off
    lmk_col = np.full(w.n_lmk, -1)
    n_obs = np.diff(w.lmk_obs_ptr)
    for l in range(w.n_lmk):
        if not lc[l] and n_obs[l] > 0 and lmk_red[l] < 0:
            lmk_col[l] = off; off += 3
    return {"dpf": dpf, "kf_off": kf_off, "lmk_red": lmk_red, "lmk_col": lmk_col, "Nr": Nr, "N": off}


def reduced_np(w):
    """N_p: the dimension of the reduced system S y = g of the window."""
    return layout(w)["Nr"]


def half_bandwidth(w):
    """The largest span, in free key-frame index, of one landmark's observations and of the IMU pairs (plan_solve's hb)."""
    kc = np.asarray(w.kf_const).astype(bool)
    fidx = np.where(kc, -1, np.cumsum(~kc) - 1)
    hb = 0
    for l in range(w.n_lmk):
        f = fidx[w.obs_kf[w.lmk_obs_ptr[l]:w.lmk_obs_ptr[l + 1]]]
        f = f[f >= 0]
        if len(f):
            hb = max(hb, int(f.max() - f.min()))
    for f in (getattr(w, "imu_factors", None) or []):
        fi, fj = fidx[int(f["kf_i"])], fidx[int(f["kf_j"])]
        if fi >= 0 and fj >= 0:
            hb = max(hb, abs(int(fi) - int(fj)))
    return hb


def band_rows(w):
    """BigPlan::bw of the window: rows below a block column of S that can be non-zero; N_p under a dense prior."""
    lay = layout(w)
    if getattr(w, "dense_prior", None) is not None:
        return lay["Nr"]
    return min(lay["Nr"], (half_bandwidth(w) + 1) * lay["dpf"])


def expected_route(Np, dpf, bw, n_win=1, band_c=0, no_bcr=False):
    """BigPlan::choose (solve_driver.h) restated: "lds" or the out-of-LDS route of a window."""
    if Np <= MAX_LDS_NP:
        return "lds"
    nb = 6 if dpf == 6 else 5
    if not (bw < Np and bw + nb <= MAX_LDS_NP):
        return "wide" if Np >= 2 * WD else "panel"
    Cw = max(nb, (MAX_LDS_NP - bw) // nb * nb)
    if band_c > 0:
        Cw = max(nb, min(Cw, band_c // nb * nb))
    Kb = (Np + bw - 1) // bw
    if nb == 6 and Kb >= 22 and 2 * bw <= MAX_LDS_NP - 1 and n_win == 1 and not no_bcr:
        return "bcr"
    return "band_twisted" if Np - bw >= 4 * Cw else "band"


def free_kf_observations(w):
    """Observation count of every free key-frame."""
    kc = np.asarray(w.kf_const).astype(bool)
    return np.bincount(w.obs_kf, minlength=w.n_kf)[~kc]


# ---- the oracle's un-reduced system -------------------------------------------------------------------------------------------------
def oracle_system(oracle_lib, w, opts):
    """(H_full, g_full) of oracle_first_step, the window's dense prior included."""
    from oracle import structs as S
    o = S.options_from(opts)
    P, keep = oracle_lib.make_problem(w, getattr(w, "dense_prior", None))
    dp_ = C.POINTER(C.c_double)
    one = np.zeros(1)
    N = oracle_lib.lib().oracle_first_step(C.byref(P), C.byref(o), dp_(), dp_(), one.ctypes.data_as(dp_), one.ctypes.data_as(dp_), -1)
    assert N == layout(w)["N"], (N, layout(w)["N"])
    H = np.zeros((N, N)); g = np.zeros(N)
    rc = oracle_lib.lib().oracle_first_step(C.byref(P), C.byref(o), dp_(), dp_(), H.ctypes.data_as(dp_), g.ctypes.data_as(dp_), N)
    assert rc == 0, rc
    return H, g


def oracle_step(oracle_lib, w, opts1):
    """The oracle's float64 first step: one iteration of oracle_solve (compute_step on the linearisation at x = 0), which also gives
    dv / dba / dbg, the kept landmarks and the trace row."""
    r = oracle_lib.solve(w, opts1, dense_prior=getattr(w, "dense_prior", None))
    assert r["summary"].num_successful_steps == 1, "the oracle rejects the first step: the window is not well posed"
    return r


# ---- the 50-digit solve ---------------------------------------------------------------------------------------------------------------
def _mpf(v):
    import mpmath
    return v if isinstance(v, mpmath.mpf) else mpmath.mpf(float(v))


def mp_envelope_cholesky_solve(A, b):
    """y of A y = b for the symmetric positive definite A (list of rows of mpf, lower triangle read) by an envelope Cholesky: row i
    of L starts at first[i], the first non-zero column of row i of A."""
    import mpmath
    n = len(b)
    first = [next(j for j in range(i + 1) if A[i][j] != 0) for i in range(n)]
    L = [[mpmath.mpf(0)] * (i + 1) for i in range(n)]
    for i in range(n):
        fi = first[i]
        for j in range(fi, i + 1):
            k0 = max(fi, first[j])
            s = A[i][j] - (mpmath.fdot(L[i][k0:j], L[j][k0:j]) if j > k0 else 0)
            if i == j:
                assert s > 0, "not positive definite"
                L[i][j] = mpmath.sqrt(s)
            else:
                L[i][j] = s / L[j][j]
    z = [mpmath.mpf(0)] * n
    for i in range(n):
        fi = first[i]
        z[i] = (b[i] - mpmath.fdot(L[i][fi:i], z[fi:i])) / L[i][i]
    y = list(z)
    for i in range(n - 1, -1, -1):       # column sweep: y_i final, then subtract its column of L^T from the rows above
        y[i] = y[i] / L[i][i]
        yi = y[i]
        for k in range(first[i], i):
            y[k] -= L[i][k] * yi
    return y


def mp_solve_system(H, g, Nr, opts, digits=50):
    """y (list of mpf) of (H + D2) y = g and the list D2, for the arrowhead H = [[Hpp, Hpl], [Hlp, blockdiag 3 x 3]] whose first Nr
    columns are the reduced part. H, g: float64 arrays (exact inputs) or object arrays of mpf."""
    import mpmath
    mpmath.mp.dps = digits
    H = np.asarray(H); g = np.asarray(g)
    N = H.shape[0]
    Hf = H.astype(np.float64)
    radius = mpmath.mpf(opts.initial_trust_region_radius)
    lo, hi = mpmath.mpf(opts.min_lm_diagonal), mpmath.mpf(opts.max_lm_diagonal)
    D2 = []
    for i in range(N):
        d = _mpf(H[i, i])
        s2 = (1 / (1 + mpmath.sqrt(d))) ** 2 if opts.jacobi_scaling else mpmath.mpf(1)
        D2.append(min(max(s2 * d, lo), hi) / radius / s2)
    gm = [_mpf(v) for v in g]
    S = [[_mpf(H[i, j]) if Hf[i, j] != 0.0 else mpmath.mpf(0) for j in range(i + 1)] for i in range(Nr)]
    for i in range(Nr):
        S[i][i] += D2[i]
    rhs = gm[:Nr]
    recs = []
    for c in range(Nr, N, 3):
        assert not np.any(Hf[c:c + 3, Nr:c]) and not np.any(Hf[c:c + 3, c + 3:]), "landmark blocks must not couple"
        M = mpmath.matrix(3, 3)
        for a in range(3):
            for b in range(3):
                M[a, b] = _mpf(H[c + a, c + b])
            M[a, a] += D2[c + a]
        Mi = mpmath.inverse(M)
        rows = [int(r) for r in np.flatnonzero(np.any(Hf[:Nr, c:c + 3] != 0.0, axis=1))]
        B = [[_mpf(H[r, c + a]) for a in range(3)] for r in rows]
        BM = [[mpmath.fdot(Br, [Mi[a, b] for a in range(3)]) for b in range(3)] for Br in B]       # B M^-1
        gl = gm[c:c + 3]
        for x, r in enumerate(rows):
            rhs[r] -= mpmath.fdot(BM[x], gl)
            for z, q in enumerate(rows):
                if q <= r:
                    S[r][q] -= mpmath.fdot(BM[x], B[z])
        recs.append((c, Mi, rows, B))
    y = mp_envelope_cholesky_solve(S, rhs) if Nr else []
    for c, Mi, rows, B in recs:
        t = [gm[c + a] - mpmath.fdot([Br[a] for Br in B], [y[r] for r in rows]) for a in range(3)]
        y += [mpmath.fdot([Mi[a, b] for b in range(3)], t) for a in range(3)]
    return y, D2, gm


def _scatter(w, lay, y):
    """The step -y as per-key-frame / per-landmark float64 arrays (the device's get_deltas layout) and as mpf arrays."""
    import mpmath
    z = mpmath.mpf(0)
    out = {k: np.full((w.n_kf, n), z, dtype=object) for k, n in (("pose", 6), ("dv", 3), ("dba", 3), ("dbg", 3))}
    out["lmk"] = np.full((w.n_lmk, 3), z, dtype=object)
    for k in range(w.n_kf):
        o = lay["kf_off"][k]
        if o < 0:
            continue
        out["pose"][k] = [-v for v in y[o:o + 6]]
        if lay["dpf"] == 15:
            out["dv"][k] = [-v for v in y[o + 6:o + 9]]; out["dba"][k] = [-v for v in y[o + 9:o + 12]]; out["dbg"][k] = [-v for v in y[o + 12:o + 15]]
    for l in range(w.n_lmk):
        o = lay["lmk_red"][l] if lay["lmk_red"][l] >= 0 else lay["lmk_col"][l]
        if o >= 0:
            out["lmk"][l] = [-v for v in y[o:o + 3]]
    return out


def _to_f64(a):
    return np.array([float(v) for v in a.ravel()], dtype=np.float64).reshape(a.shape)


def mp_candidate_cost(w, step_mp, digits=50, huber_a=0.0):
    """Cost of the window at the 50-digit candidate (every residual block evaluated by the twin in 50-digit arithmetic, under the
    Huber loss of the visual factors if huber_a > 0)."""
    from oracle import twin
    B = twin.Backend("mp", digits)
    P = twin.Problem(B, w, huber_a=huber_a)
    x = B.zeros(P.n)
    for k in range(w.n_kf):
        if P.kf_col[k] >= 0:
            x[P.kf_col[k]:P.kf_col[k] + 6] = step_mp["pose"][k]
            if P.has_imu:
                x[P.v_col[k]:P.v_col[k] + 3] = step_mp["dv"][k]; x[P.ba_col[k]:P.ba_col[k] + 3] = step_mp["dba"][k]
                x[P.bg_col[k]:P.bg_col[k] + 3] = step_mp["dbg"][k]
    for l in range(w.n_lmk):
        if P.lmk_col[l] >= 0:
            x[P.lmk_col[l]:P.lmk_col[l] + 3] = step_mp["lmk"][l]
    cost, _, _, _ = P.evaluate(x, want_j=False)
    return float(cost)


def mp_first_step(w, opts, digits=50, system=None, oracle_lib=None, want_cost=True):
    """The 50-digit first LM step of the window, rounded to float64 at the end: {"pose", "dv", "dba", "dbg" [n_kf, .], "lmk" [n_lmk, 3],
    "model_cost_change", "cost" (after the step; None unless want_cost), "mp": the same fields before the rounding}. system: (H_full, g_full) in the oracle's ordering instead of the
    oracle's own (float64, or mpf for the check against the twin)."""
    import mpmath
    mpmath.mp.dps = digits
    lay = layout(w)
    if system is None:
        if oracle_lib is None:
            from oracle import oracle as oracle_lib
        system = oracle_system(oracle_lib, w, opts)
    H, g = system
    assert np.asarray(H).shape[0] == lay["N"]
    y, D2, gm = mp_solve_system(H, g, lay["Nr"], opts, digits)
    mcc = (mpmath.fdot(y, gm) + mpmath.fdot([a * a for a in y], D2)) / 2
    step = _scatter(w, lay, y)
    out = {k: _to_f64(v) for k, v in step.items()}
    out["model_cost_change"] = float(mcc)
    out["cost"] = mp_candidate_cost(w, step, digits, huber_a=float(opts.huber_a)) if want_cost else None
    out["mp"] = dict(step, model_cost_change=mcc)
    return out


# ---- the metric -----------------------------------------------------------------------------------------------------------------------
def pose_part(d, w):
    """The pose step of the free key-frames with the dv / dba / dbg columns of a VIO window: [n_free, 6 or 15]."""
    free = ~np.asarray(w.kf_const).astype(bool)
    cols = [d["pose"][free]]
    if int(getattr(w, "has_imu", 0)):
        cols += [d["dv"][free], d["dba"][free], d["dbg"][free]]
    return np.concatenate(cols, axis=1)


def step_error(got, ref, w):
    """(pose part, landmark part) of max |got - ref| / max |ref|."""
    gp, rp = pose_part(got, w), pose_part(ref, w)
    return (float(np.abs(gp - rp).max() / np.abs(rp).max()), float(np.abs(got["lmk"] - ref["lmk"]).max() / np.abs(ref["lmk"]).max()))


def bars(case):
    """(pose bar, landmark bar) of a case: TOL_FACTOR x max(E_REF, FLOOR)."""
    e = E_REF[case.window]
    return TOL_FACTOR * max(e[0], FLOOR), TOL_FACTOR * max(e[1], FLOOR)


# ---- the float64 host model of the blocked Cholesky solve, with planted defects ---------------------------------------------------------
def reduced_system_f64(H, g, Nr, opts, no_damping_on=None, li_hook=None):
    """(S, rhs, Li [L, 3, 3], D2) of the float64 Schur complement of the oracle's system (NumPy). li_hook(M, Li) may replace the
    inverse Cholesky factors of the landmark blocks (a planted defect)."""
    N = H.shape[0]
    d = np.diag(H).copy()
    s2 = (1.0 / (1.0 + np.sqrt(d))) ** 2 if opts.jacobi_scaling else np.ones(N)
    D2 = np.clip(s2 * d, opts.min_lm_diagonal, opts.max_lm_diagonal) / opts.initial_trust_region_radius / s2
    if no_damping_on is not None:
        D2 = D2.copy(); D2[no_damping_on] = 0.0
    L = (N - Nr) // 3
    S = H[:Nr, :Nr] + np.diag(D2[:Nr])
    rhs = g[:Nr].copy()
    Li = np.zeros((L, 3, 3))
    if L:
        # the elimination in Cholesky form, as the oracle and the device do it: M = Lc Lc^T, Li = Lc^-1, W = B Li^T, S -= W W^T
        idx = Nr + 3 * np.arange(L)
        M = np.stack([H[c:c + 3, c:c + 3] + np.diag(D2[c:c + 3]) for c in idx])
        Li = np.linalg.inv(np.linalg.cholesky(M))
        if li_hook is not None:
            Li = li_hook(M, Li)
        Bm = H[:Nr, Nr:].reshape(Nr, L, 3)
        W = np.einsum("rla,lba->rlb", Bm, Li).reshape(Nr, 3 * L)
        S = S - W @ W.T
        rhs = rhs - W @ np.einsum("lab,lb->la", Li, g[Nr:].reshape(L, 3)).ravel()
    return S, rhs, Li, D2


def back_substitute_f64(H, g, Nr, Li, yp):
    L = (H.shape[0] - Nr) // 3
    if not L:
        return np.zeros(0)
    t = g[Nr:] - H[Nr:, :Nr] @ yp
    u = np.einsum("lab,lb->la", Li, t.reshape(L, 3))
    return np.einsum("lba,lb->la", Li, u).ravel()


RSQ_SEED_ERROR = 2.0 ** -24      # v_rsq_f64 before its refinement


def blocked_cholesky_solve(S, rhs, rsq_defect_at=None, drop_product=False, _live=None):
    """Float64 host model of the in-LDS solve (chol16.h): the (N + 1)-row matrix [S; rhs^T] on 16 x 16 tiles, right-looking over block
    columns, 4-column steps inside a block column (the 4 x 4 pivot block by reciprocal square roots, then ONE rank-4 product on
    the rest of the block column), four rank-4 products per trailing tile, the forward substitution in the rhs row, and a
    back-substitution that multiplies by the pivots' reciprocal square roots as the factorisation does. Not the MFMA lane layout: the same sums in the same blocking.
    rsq_defect_at = j: pivot j's reciprocal square root carries the relative error of the unrefined hardware seed.
    drop_product: the last rank-4 product of ONE trailing tile update is dropped: tile (rhs tile row, last real block column) in the
    update by the block column before it; in a one-tile system (N < 16) the last in-tile rank-4 product that reaches a real column
    with an operand that is not structurally zero (the bias columns of a lone VIO key-frame couple to nothing)."""
    N = len(rhs)
    nb = (N + 1 + 15) // 16
    A = np.zeros((16 * nb, 16 * nb))
    A[:N, :N] = np.tril(S)
    A[N, :N] = rhs
    Jd = (N - 1) >> 4                                    # last real block column
    step_d = -1
    if drop_product and Jd == 0:                         # one tile: the last step whose product changes a column < N
        live = []
        blocked_cholesky_solve(S, rhs, _live=live)
        step_d = live[-1]
    invs = np.zeros(N)                                   # the device never divides: both substitutions multiply by these
    for k in range(nb):
        c0, c1 = 16 * k, min(16 * k + 16, N)
        for s in range(4):
            j0, j1 = c0 + 4 * s, min(c0 + 4 * s + 4, N)
            if j0 >= N:
                break
            for j in range(j0, j1):                      # the 4 x 4 pivot block and the step's columns of every row below
                inv = 1.0 / np.sqrt(A[j, j])
                if rsq_defect_at == j:
                    inv *= 1.0 + RSQ_SEED_ERROR
                invs[j] = inv
                A[j:N + 1, j] *= inv
                for c in range(j + 1, j1):
                    A[c:N + 1, c] -= A[c:N + 1, j] * A[c, j]
            if j1 < c1 and not (drop_product and Jd == 0 and s == step_d):   # the rank-4 product on the rest of the block column
                Y = A[j1:N + 1, j0:j1]
                if _live is not None and k == 0 and np.any(Y[:c1 - j1] != 0.0):
                    _live.append(s)
                A[j1:N + 1, j1:c1] -= Y @ Y[:c1 - j1].T
        if c1 < N:                                       # trailing update, 4 rank-4 products per tile
            for q in range(4):
                Yq = A[c0 + 16:N + 1, c0 + 4 * q:c0 + 4 * q + 4]
                A[c0 + 16:N + 1, c0 + 16:N] -= Yq @ Yq[:N - c0 - 16].T
                if drop_product and q == 3 and Jd >= 1 and k == Jd - 1:      # undo it on the one tile
                    r0, cj0, cj1 = 16 * (nb - 1), 16 * Jd, min(16 * Jd + 16, N)
                    A[r0:N + 1, cj0:cj1] += A[r0:N + 1, c0 + 12:c0 + 16] @ A[cj0:cj1, c0 + 12:c0 + 16].T
    Lf = np.tril(A[:N, :N])
    y = A[N, :N].copy()
    for i in range(N - 1, -1, -1):
        y[i] = (y[i] - Lf[i + 1:, i] @ y[i + 1:]) * invs[i]
    return y


def host_model_step(w, H, g, opts, defect=None):
    """The float64 step of the host model in get_deltas layout. defect: None, ("rsq", j), "product" or "damping"."""
    lay = layout(w)
    Nr = lay["Nr"]
    S, rhs, Minv, D2 = reduced_system_f64(H, g, Nr, opts)
    if defect == "damping":
        S[Nr - 1, Nr - 1] -= D2[Nr - 1]
    yp = blocked_cholesky_solve(S, rhs, rsq_defect_at=defect[1] if isinstance(defect, tuple) else None, drop_product=defect == "product")
    y = np.concatenate([yp, back_substitute_f64(H, g, Nr, Minv, yp)])
    return {k: v.astype(np.float64) for k, v in _scatter(w, lay, list(y)).items()}


# ---- the float64 host model of the tile kernels, with planted defects ------------------------------------------------------------------
def _chol3_inverse_with_rsq_error(M, rel):
    """Lc^-1 of the 3 x 3 block M = Lc Lc^T, by reciprocal square roots as the tile kernels form it, the FIRST pivot's carrying the
    relative error rel."""
    i0 = (1.0 + rel) / np.sqrt(M[0, 0])
    l10, l20 = M[1, 0] * i0, M[2, 0] * i0
    i1 = 1.0 / np.sqrt(M[1, 1] - l10 * l10)
    l21 = (M[2, 1] - l20 * l10) * i1
    i2 = 1.0 / np.sqrt(M[2, 2] - l20 * l20 - l21 * l21)
    a10 = -l10 * i0 * i1
    a21 = -l21 * i1 * i2
    a20 = -(l20 * i0 + l21 * a10) * i2
    return np.array([[i0, 0.0, 0.0], [a10, i1, 0.0], [a20, a21, i2]])


TILE_DEFECTS = ("observation scaled by 1 + 2^-24", "rsq seed on a landmark's first pivot", "a Jp dp term missing from the back-substitution",
                "E M^-1 g_l of a landmark missing from the reduced gradient")


def tile_host_model_step(w, opts, defect=None, lanes=256):
    """The float64 step of a host model of the tile kernels, in get_deltas layout: the un-reduced system summed observation by
    observation from the twin's float64 Jacobian rows (oracle/twin.py: not the oracle's linearisation), the landmark blocks
    eliminated in Cholesky form (reduced_system_f64), the reduced system solved by LAPACK, the landmarks back-substituted.
    defect: None or one of TILE_DEFECTS, planted on a landmark / observation chosen from the window's shape:
      - the rows of Jp, Jl and r of ONE observation scaled by 1 + 2^-24: an unrefined 1 / z in one lane;
      - the first pivot's reciprocal square root of ONE landmark's 3 x 3 block off by 2^-24 (the hardware seed, unrefined);
      - the Jp dp term of ONE observation of the last landmark of the window's first tile missing from its back-substitution;
      - that landmark's E M^-1 g_l missing from the reduced gradient."""
    from oracle import twin
    assert defect is None or defect in TILE_DEFECTS
    lay = layout(w)
    Nr, N = lay["Nr"], lay["N"]
    B = twin.Backend("f64")
    P = twin.Problem(B, w, huber_a=float(opts.huber_a))
    assert P.n == N and not P.has_imu and np.array_equal(lay["kf_off"], P.kf_col) and np.array_equal(lay["lmk_col"], P.lmk_col)
    n_obs = len(w.obs_kf)
    lmk_of = np.repeat(np.arange(w.n_lmk), np.diff(w.lmk_obs_ptr))
    both_free = [o for o in range(n_obs) if P.kf_col[w.obs_kf[o]] >= 0 and P.lmk_col[lmk_of[o]] >= 0]
    G = 8
    while G < np.diff(w.lmk_obs_ptr).max():
        G *= 2
    # last landmark of the first tile (contiguous cut, one round) that a free key-frame observes
    l_last = max(int(l) for l in lmk_of[both_free] if l < min(lanes // G, w.n_lmk))
    o_last = next(o for o in both_free if lmk_of[o] == l_last)
    o_mid = both_free[len(both_free) // 2]
    l_rsq = lmk_of[both_free[len(both_free) // 3]]
    H = np.zeros((N, N)); g = np.zeros(N)
    J_last = None
    for b, (r, cols, inprog, _) in enumerate(P.blocks(B.zeros(P.n))):
        if not inprog:
            continue
        if defect == TILE_DEFECTS[0] and b == o_mid:
            f = 1.0 + 2.0 ** -24
            r, cols = f * r, [(c, f * Jb) for c, Jb in cols]
        if b == o_last:
            J_last = dict(cols)
        for ca, Ja in cols:
            g[ca:ca + Ja.shape[1]] += Ja.T @ r
            for cb, Jb in cols:
                H[ca:ca + Ja.shape[1], cb:cb + Jb.shape[1]] += Ja.T @ Jb
    hook = None
    if defect == TILE_DEFECTS[1]:
        def hook(M, Li):
            Li = Li.copy()
            i = (lay["lmk_col"][l_rsq] - Nr) // 3
            assert np.abs(_chol3_inverse_with_rsq_error(M[i], 0.0) - Li[i]).max() <= 1e-8 * np.abs(Li[i]).max()     # the same factor
            Li[i] = _chol3_inverse_with_rsq_error(M[i], RSQ_SEED_ERROR)
            return Li
    S, rhs, Li, D2 = reduced_system_f64(H, g, Nr, opts, li_hook=hook)
    c_last = lay["lmk_col"][l_last]
    if defect == TILE_DEFECTS[3]:
        i = (c_last - Nr) // 3
        rhs = rhs + H[:Nr, c_last:c_last + 3] @ (Li[i].T @ (Li[i] @ g[c_last:c_last + 3]))
    yp = np.linalg.solve(S, rhs)
    Hb = H
    if defect == TILE_DEFECTS[2]:
        kc = P.kf_col[w.obs_kf[o_last]]
        Hb = H.copy()
        Hb[c_last:c_last + 3, kc:kc + 6] -= J_last[c_last].T @ J_last[kc]
    y = np.concatenate([yp, back_substitute_f64(Hb, g, Nr, Li, yp)])
    return {k: v.astype(np.float64) for k, v in _scatter(w, lay, list(y)).items()}


# ---- the cases ------------------------------------------------------------------------------------------------------------------------
PIXEL, ANGULAR = capi.FACTOR_PIXEL, capi.FACTOR_ANGULAR
LMK_PER_KF = 12
MAX_OBS_PER_LMK = 64              # the library's limit (set_windows)
GOLDEN_FROM_NP = 96               # from here on the 50-digit evaluation of the candidate cost alone takes more than a few seconds
SPREAD = 2                        # make_window's band: a landmark seeded in key-frame k is seen from k - 2 .. k + 2, so every key-frame is observed


@dataclasses.dataclass
class Case:
    name: str
    np_: int                      # N_p the window is built for
    route: str                    # "lds", "lds_extras" or the out-of-LDS route it is meant to take
    build: object                 # () -> window
    env: dict = dataclasses.field(default_factory=dict)
    golden: bool = False          # the reference is read from tests/golden/first_step_ref.npz
    window: str = ""              # key of the window (cases that differ in their switches only share a window and a reference)
    opts: dict = dataclasses.field(default_factory=dict)    # fields of the solve options other than gn_options(1)'s: {"huber_a": a}
    front: tuple = ()             # decoys of batch_helpers stored in front of the window in one batch
    kernels: str = ""             # "latency" / "throughput" / "pf": the kernels the GPU test asserts from kernel_times() ("": not asserted)
    plan: dict = None             # what layout_plan.h must make of the window under the case's switches (tests/test_tile_plan_cpu.py)

    def __post_init__(self):
        self.window = self.window or self.name
        self.golden = self.golden or self.np_ >= GOLDEN_FROM_NP


def case_options(case, iters=1):
    """gn_options(iters) with the case's options."""
    o = capi.gn_options(iters)
    for k, v in case.opts.items():
        setattr(o, k, v)
    return o


def vo_window(free, factor=PIXEL, band=SPREAD, seed=None):
    n_kf = free + 1
    return synthetic.make_window(n_kf=n_kf, n_lmk=LMK_PER_KF * n_kf, obs_per_lmk=4, seed=7000 + free if seed is None else seed, factor=factor,
                                 band=band)


def vio_window(free, band=SPREAD):
    from vio_helpers import make_vio_window
    n_kf = free + 1
    return make_vio_window(n_kf=n_kf, n_lmk=LMK_PER_KF * n_kf, obs_per_lmk=4, seed=7100 + free, fixed=1, band=band)


def kept_window(free, n_keep, vio):
    """free key-frames and n_keep kept landmarks under a full-rank dense prior (on the oldest free key-frame's 15 states too, VIO)."""
    from test_gpu_prior import random_prior
    w = vio_window(free) if vio else vo_window(free, seed=7200 + free)
    w.dense_prior = random_prior(w, n_keep, w.n_kf - 2 if vio else -1, np.random.default_rng(7300 + free), rank_deficit=0)
    return w


def dense_vo_window(free):
    """A VO window whose reduced system is dense (bw = N_p): narrow tracks and, between them, one landmark seen by every view (as
    cov_helpers.window_obs64; the key-frames stand close enough for one point to be in every view)."""
    import cov_helpers as ch
    n_kf = free + 1
    kw = dict(n_kf=n_kf, seed=7400 + free, length=4.0)
    a = synthetic.make_window(n_lmk=LMK_PER_KF * n_kf, obs_per_lmk=4, band=SPREAD, **kw)
    b = synthetic.make_window(n_lmk=1, obs_per_lmk=2 * n_kf, **kw)
    assert np.array_equal(a.kf_T_f_w[a.kf_const == 1], b.kf_T_f_w[b.kf_const == 1])
    sel = np.arange(2 * n_kf)
    if len(sel) > MAX_OBS_PER_LMK:                       # keep every key-frame, drop the second camera of some in the middle
        drop = 2 * (n_kf // 2 + np.arange(len(sel) - MAX_OBS_PER_LMK)) + 1
        sel = np.setdiff1d(sel, drop)
    h = a.n_lmk // 2
    return ch._assemble(a, [(a, l, None) for l in range(h)] + [(b, 0, sel)] + [(a, l, None) for l in range(h, a.n_lmk)])


# every switch a case may set (the handle reads them once, in create): a test clears them all, so that nothing leaks between cases
SWITCHES = ("SADVIO_BAND_C", "SADVIO_NO_BCR", "SADVIO_LM", "SADVIO_TILE_ROUNDS", "SADVIO_LM_SUBS", "SADVIO_CONTIG_TILES", "SADVIO_NO_PRE",
            "SADVIO_PF_WG", "SADVIO_IMU_ITEMS")


# ---- windows of the tile-kernel variants (k_build / k_backsub of kernels.h, k_lm_pass0 / k_build_obs / k_lm_pass of lm_kernels.h) ---------
HUBER_A = 1.345 ** 0.5
SMALL_PERTURB = dict(rot_perturb_deg=0.02, trans_perturb=0.001, lmk_perturb=0.002)   # leaves part of the residuals inside the Huber threshold


def w70(factor=PIXEL, const=False, small=False):
    """W70: 4 key-frames (3 free), 70 landmarks of 5 observations: chunks of 12 landmarks = 60 lanes. const: key-frame 1 (in the
    middle of every tile's list) and every seventh landmark constant."""
    w = synthetic.make_window(n_kf=4, n_lmk=70, obs_per_lmk=5, seed=7500, factor=factor, **(SMALL_PERTURB if small else {}))
    if const:
        w.kf_const = w.kf_const.copy(); w.kf_const[1] = 1
        w.lmk_const = np.zeros(w.n_lmk, dtype=np.uint8); w.lmk_const[::7] = 1
    return w


def wide_group_window(n_kf, n_lmk, obs_per_lmk, seed, **kw):
    """Landmarks of more than 8 observations (16 / 32 / 64 lanes each). All but 5 key-frames are constant: a tile of more than 5
    free key-frames ends at its first landmark (layout_tiles' soft limit), and these tiles are to be full."""
    return synthetic.make_window(n_kf=n_kf, n_lmk=n_lmk, obs_per_lmk=obs_per_lmk, seed=seed, fixed=max(1, n_kf - 5), **kw)


def free6_window():
    """40 narrow tracks over 8 key-frames and, between them, 2 landmarks seen once from each of 6 free key-frames: G = 8 tiles of 6
    free key-frames (lds_mode 1) beside the MFMA tiles of the narrow tracks."""
    import test_gpu_tile_packing as tp
    a, b = tp._pair(8, 40, 60, 7716)
    wd = tp._wide(b, 0, 6, n=6)
    assert len(wd) >= 2
    return tp._insert(a, {12: wd[0:1], 30: wd[1:2]})


LM_MIXED_COUNTS = (8, 7, 8, 6, 8, 8, 7, 8, 5, 2, 3, 4, 2, 5, 3, 2, 4, 3, 2, 5, 4, 6, 8, 2, 7, 3, 8, 8, 4, 6, 2, 2, 3, 5, 8, 7, 6, 8, 8, 3, 2, 2, 4, 2, 3, 2, 2, 3, 2, 4)


def lm_mixed_window():
    """Landmarks of 2 .. 8 observations in an irregular order: the first LM_MIXED_COUNTS[l] observations of the landmarks of an
    8-observation window."""
    import cov_helpers as ch
    a = synthetic.make_window(n_kf=4, n_lmk=len(LM_MIXED_COUNTS), obs_per_lmk=8, seed=7600)
    return ch._assemble(a, [(a, l, np.arange(n)) for l, n in enumerate(LM_MIXED_COUNTS)])


def chunk_cuts(counts, tile=32, chunk=12, lanes=64):
    """layout_chunks restated for tiles of `tile` consecutive landmarks: [(landmarks, observations, what closed the chunk)] with
    "obs" (the next landmark would pass 64 observations), "lmk" (12 landmarks) or "tile" (the tile ends)."""
    out, l = [], 0
    while l < len(counts):
        end = min(l - l % tile + tile, len(counts))
        nl = no = 0
        while l < end and nl < chunk and no + counts[l] <= lanes:
            no += counts[l]; nl += 1; l += 1
        out.append((nl, no, "tile" if l == end else "lmk" if nl == chunk else "obs"))
    return out


def beyond_huber(w, a=HUBER_A):
    """Share of the observations whose residual norm at x = 0 exceeds the Huber threshold (the twin's residuals, no loss)."""
    from oracle import twin
    B = twin.Backend("f64")
    P = twin.Problem(B, w)
    n = [float(np.hypot(r[0], r[1])) for (r, _, _, _), _ in zip(P.blocks(B.zeros(P.n), want_j=False), range(len(w.obs_kf)))]
    return float(np.mean(np.array(n) > a))


# ---- the planner's input (tests/cpp/dump_tile_plan.cpp) --------------------------------------------------------------------------------
def plan_input(ws, env):
    """The track structure of the windows and the LayoutIn switches of a case's environment, as dump_tile_plan reads them."""
    num = lambda k, d: int(env.get(k, d))
    out = [f"{num('SADVIO_LM', -1)} {num('SADVIO_TILE_ROUNDS', 0)} {num('SADVIO_LM_SUBS', 0)} {num('SADVIO_CONTIG_TILES', 0)} {num('SADVIO_NO_PRE', 0)}",
           str(len(ws))]
    for w in ws:
        lc = np.zeros(w.n_lmk, int) if getattr(w, "lmk_const", None) is None else np.asarray(w.lmk_const).astype(int)
        out.append(f"{w.n_kf} {len(w.cam_sigma)} {int(getattr(w, 'has_imu', 0))} {w.n_lmk}")
        out.append(" ".join(str(int(v)) for v in w.kf_const))
        out.append(" ".join(str(v) for v in lc))
        for l in range(w.n_lmk):
            o = range(w.lmk_obs_ptr[l], w.lmk_obs_ptr[l + 1])
            out.append(" ".join([str(len(o))] + [f"{int(w.obs_kf[i])} {int(w.obs_cam[i])}" for i in o]))
    return "\n".join(out) + "\n"


def parse_plan(text):
    """dump_tile_plan's output: {"lm_ok", "lm_ksub", "lm_n_sub", "pre_ok", "gemm_run4", "tiles": [{"w", "lds_mode", "G", "n_lmk",
    "n_free", "n_kf", "packed", "chunks": [(landmarks, observations)]}]}."""
    plan = {"tiles": []}
    for line in text.splitlines():
        v = line.split()
        if v[0] == "P":
            plan.update(zip(("lm_ok", "lm_ksub", "lm_n_sub", "pre_ok", "gemm_run4", "n_tiles"), map(int, v[1:])))
        elif v[0] == "T":
            n = [int(x) for x in v[1:]]
            t = dict(zip(("w", "lds_mode", "G", "n_lmk", "n_free", "n_kf", "packed"), n[1:8]))
            t["chunks"] = [(n[9 + 2 * i], n[10 + 2 * i]) for i in range(n[8])]
            plan["tiles"].append(t)
    assert plan["n_tiles"] == len(plan["tiles"])
    return plan


def case_windows(case):
    """The windows of the case's batch: its decoys, then its window."""
    import batch_helpers as bh
    w = case_window(case)
    return [bh.decoy(w.factor_type, d) for d in case.front] + [w]


def _cases():
    out = []
    star = {3, 8, 19, 29}
    for free in (1, 2, 3, 5, 8, 16, 18, 19, 24, 28, 29):
        out.append(Case(f"vo{6 * free}", 6 * free, "lds", lambda f=free: vo_window(f)))
        if free in star:
            out.append(Case(f"vo{6 * free}_angular", 6 * free, "lds", lambda f=free: vo_window(f, ANGULAR)))
    for free in (1, 2, 11):
        out.append(Case(f"vio{15 * free}", 15 * free, "lds_extras", lambda f=free: vio_window(f)))
    for free, keep, vio in ((3, 6, True), (18, 1, False), (26, 1, False), (11, 3, True)):
        n = (15 if vio else 6) * free + 3 * keep
        out.append(Case(f"kept{n}", n, "lds_extras", lambda f=free, k=keep, v=vio: kept_window(f, k, v)))
    for free, route in ((30, "panel"), (31, "panel"), (32, "wide"), (33, "wide")):
        out.append(Case(f"dense{6 * free}", 6 * free, route, lambda f=free: dense_vo_window(f), golden=True))
    band = lambda f: vo_window(f, band=1)
    out.append(Case("band180", 180, "band", lambda: band(30), golden=True))
    out.append(Case("band342", 342, "band", lambda: band(57), golden=True))
    out.append(Case("band180_vio", 180, "band", lambda: vio_window(12, band=1), golden=True))
    out.append(Case("twisted180", 180, "band_twisted", lambda: band(30), env={"SADVIO_BAND_C": "12"}, golden=True, window="band180"))
    out.append(Case("twisted186", 186, "band_twisted", lambda: band(31), env={"SADVIO_BAND_C": "12"}, golden=True))
    out.append(Case("band378", 378, "band", lambda: band(63), golden=True))                 # 21 blocks: one short of bcr
    for free in (64, 67, 97):                                                                 # 22, 23 (odd), 33 (2^5 + 1) blocks
        n = 6 * free
        out.append(Case(f"bcr{n}", n, "bcr", lambda f=free: band(f), golden=True))
        # without bcr these lengths stay below 4 C at the default window: the one-sided band solver takes them
        out.append(Case(f"nobcr{n}", n, "band", lambda f=free: band(f), env={"SADVIO_NO_BCR": "1"}, golden=True, window=f"bcr{n}"))
    return out


def _plan(tiles, packed=0, chunks=None, lm_ok=0, lm_ksub=1, lm_n_sub=0, pre_ok=1):
    """tiles: (lds_mode, G, landmarks, free key-frames) of the window's tiles in order; chunks: per tile [(landmarks, observations)]."""
    return dict(tiles=tiles, packed=packed, chunks=chunks, lm_ok=lm_ok, lm_ksub=lm_ksub, lm_n_sub=lm_n_sub, pre_ok=pre_ok)


def _tile_cases():
    """One case per variant of the tile kernels (ISSUE: the first LM step of every tile-kernel variant). All windows are small: the
    in-LDS k_solve solves them, and the 50-digit reference costs seconds."""
    out = []
    T3 = [(2, 8, 32, 2), (2, 8, 32, 3), (2, 8, 6, 3)]         # W70 in single-round tiles
    C3 = [[(12, 60), (12, 60), (8, 40)], [(12, 60), (12, 60), (8, 40)], [(6, 30)]]
    C1 = [[(12, 60)] * 5 + [(10, 50)]]
    lat = lambda name, np_, build, plan, env=None, **kw: out.append(Case(name, np_, "lds", build, env=env or {}, kernels="latency", plan=plan, **kw))
    lm = lambda name, np_, build, plan, env=None, **kw: out.append(
        Case(name, np_, "lds", build, env=dict({"SADVIO_LM": "1"}, **(env or {})), kernels="throughput", plan=plan, **kw))
    R3 = {"SADVIO_TILE_ROUNDS": "3"}
    # the latency kernels (kernels.h)
    lat("w70", 18, w70, _plan(T3, packed=1))
    lat("w70_contig", 18, w70, _plan(T3), env={"SADVIO_CONTIG_TILES": "1"}, window="w70")
    lat("w70_nopre", 18, w70, _plan(T3, packed=1, pre_ok=0), env={"SADVIO_NO_PRE": "1"}, window="w70")
    lat("w70_rounds2", 18, w70, _plan([(2, 8, 64, 3), (2, 8, 6, 3)]), env={"SADVIO_TILE_ROUNDS": "2"}, window="w70")
    lat("w70_rounds3", 18, w70, _plan([(2, 8, 70, 3)]), env=R3, window="w70")
    const = lambda: w70(const=True)
    lat("w70_const", 12, const, _plan([(2, 8, 32, 1), (2, 8, 32, 2), (2, 8, 6, 2)], packed=1))
    lat("w70_const_rounds3", 12, const, _plan([(2, 8, 70, 2)]), env=R3, window="w70_const")
    hub = lambda: w70(small=True)
    lat("w70_huber", 18, hub, _plan(T3, packed=1), opts={"huber_a": HUBER_A})
    lat("w70_huber_rounds3", 18, hub, _plan([(2, 8, 70, 3)]), env=R3, opts={"huber_a": HUBER_A}, window="w70_huber")
    lat("g16", 30, lambda: wide_group_window(6, 24, 10, 7610), _plan([(1, 16, 16, 5), (1, 16, 8, 5)], packed=1))
    lat("g32", 30, lambda: wide_group_window(10, 9, 18, 7620, length=4.0), _plan([(1, 32, 8, 5), (1, 32, 1, 5)], packed=1))
    lat("g64", 30, lambda: wide_group_window(18, 6, 34, 7630, length=4.0), _plan([(1, 64, 4, 5), (1, 64, 2, 5)], packed=1))
    lat("free6", 42, free6_window, _plan([(2, 8, 32, 5), (2, 8, 8, 4), (1, 8, 1, 6), (1, 8, 1, 6)], packed=1))
    vio30 = lambda: vio_window(2)
    V2 = _plan([(2, 8, 32, 2), (2, 8, 4, 2)], packed=1)
    out.append(Case("vio30_pf", 30, "lds_extras", vio30, env={"SADVIO_PF_WG": "0"}, window="vio30", kernels="pf", plan=V2))
    out.append(Case("vio30_items", 30, "lds_extras", vio30, env={"SADVIO_IMU_ITEMS": "1"}, window="vio30", kernels="latency", plan=V2))
    # the throughput kernels (lm_kernels.h)
    ang = lambda: w70(ANGULAR)
    lm("lm70", 18, w70, _plan(T3, chunks=C3, lm_ok=1, lm_n_sub=3), window="w70")
    lm("lm70_angular", 18, ang, _plan(T3, chunks=C3, lm_ok=1, lm_n_sub=3), window="w70_angular")
    lm("lm70_rounds3", 18, w70, _plan([(2, 8, 70, 3)], chunks=C1, lm_ok=1, lm_ksub=2, lm_n_sub=1), env=R3, window="w70")
    lm("lm70_rounds3_angular", 18, ang, _plan([(2, 8, 70, 3)], chunks=C1, lm_ok=1, lm_ksub=2, lm_n_sub=1), env=R3, window="w70_angular")
    lm("lm70_rounds3_subs2", 18, w70, _plan([(2, 8, 70, 3)], chunks=C1, lm_ok=1, lm_ksub=2, lm_n_sub=1), env=dict(R3, SADVIO_LM_SUBS="2"), window="w70")
    lm("lm70_const", 12, const, _plan([(2, 8, 32, 1), (2, 8, 32, 2), (2, 8, 6, 2)], chunks=C3, lm_ok=1, lm_n_sub=3), window="w70_const")
    lm("lm_obs8", 18, lambda: synthetic.make_window(n_kf=4, n_lmk=40, obs_per_lmk=8, seed=7640),
       _plan([(2, 8, 32, 3), (2, 8, 8, 3)], chunks=[[(8, 64)] * 4, [(8, 64)]], lm_ok=1, lm_n_sub=2))
    lm("lm_mixed", 18, lm_mixed_window,
       _plan([(2, 8, 32, 3), (2, 8, 18, 3)], chunks=[[(8, 60), (12, 40), (12, 60)], [(12, 58), (6, 16)]], lm_ok=1, lm_n_sub=2))
    lm("lm_free1", 6, lambda: synthetic.make_window(n_kf=2, n_lmk=40, obs_per_lmk=4, seed=7650),
       _plan([(2, 8, 32, 1), (2, 8, 8, 1)], chunks=[[(12, 48), (12, 48), (8, 32)], [(8, 32)]], lm_ok=1, lm_n_sub=2))
    lm("lm_free5", 30, lambda: synthetic.make_window(n_kf=6, n_lmk=32, obs_per_lmk=8, seed=7661),
       _plan([(2, 8, 32, 5)], chunks=[[(8, 64)] * 4], lm_ok=1, lm_n_sub=1))
    lm("lm70@2", 18, w70, _plan(T3, chunks=C3, lm_ok=1, lm_n_sub=10), window="w70", front=("a", "b"))
    return out


OLD_CASES = _cases()              # the reduced-solve routes
TILE_CASES = _tile_cases()        # the tile-kernel variants
CASES = OLD_CASES + TILE_CASES
CASE = {c.name: c for c in CASES}
LDS_CASES = [c for c in OLD_CASES if c.route in ("lds", "lds_extras")]      # the sizes of the in-LDS Cholesky
BIG_CASES = [c for c in CASES if c.route not in ("lds", "lds_extras")]
BATCH_CASE = "vo114"              # the in-LDS window that is also solved at index 2 of a batch

_windows = {}


def case_window(case):
    """The case's window (built once per process; never modified)."""
    if case.window not in _windows:
        _windows[case.window] = case.build()
    return _windows[case.window]


_refs = {}


def reference(case, oracle_lib):
    """The 50-digit first step of the case (computed once per process, or read from the committed fixture)."""
    key = case.window
    if key in _refs:
        return _refs[key]
    w = case_window(case)
    if case.golden:
        z = np.load(GOLDEN)
        ref = {k: z[f"{key}/{k}"] for k in ("pose", "dv", "dba", "dbg", "lmk")}
        ref["model_cost_change"], ref["cost"] = float(z[f"{key}/model_cost_change"]), float(z[f"{key}/cost"])
        assert ref["pose"].shape == (w.n_kf, 6) and ref["lmk"].shape == (w.n_lmk, 3)
    else:
        ref = mp_first_step(w, case_options(case), oracle_lib=oracle_lib)
    _refs[key] = ref
    return ref


# (pose part, landmark part) of step_error(oracle float64 step, 50-digit step); measured by
# test_step_reference_cpu.py::test_e_ref_table_brackets_the_measured_values, recorded 1.5 x the measured value rounded up to two digits
# (the test accepts a recorded value between 1 x and 4 x the measured one)
E_REF = {
    "vo6": (5.7e-13, 6.7e-13),
    "vo12": (5.0e-13, 3.9e-13),
    "vo18": (1.9e-12, 8.0e-13),
    "vo18_angular": (7.9e-13, 5.6e-13),
    "vo30": (1.5e-12, 3.1e-13),
    "vo48": (8.6e-13, 2.9e-13),
    "vo48_angular": (1.5e-12, 3.4e-13),
    "vo96": (1.7e-12, 3.1e-13),
    "vo108": (2.8e-12, 5.1e-13),
    "vo114": (8.5e-13, 3.1e-13),
    "vo114_angular": (7.6e-13, 4.3e-13),
    "vo144": (3.3e-12, 2.7e-13),
    "vo168": (1.3e-12, 4.5e-13),
    "vo174": (1.1e-12, 4.4e-13),
    "vo174_angular": (1.5e-12, 4.1e-13),
    "vio15": (1.6e-14, 5.6e-14),
    "vio30": (1.3e-14, 5.3e-14),
    "vio165": (1.1e-13, 3.6e-13),
    "kept63": (6.9e-15, 6.7e-14),
    "kept111": (1.2e-12, 6.5e-13),
    "kept159": (1.2e-12, 7.0e-13),
    "kept174": (1.3e-13, 4.2e-13),
    "dense180": (4.2e-13, 2.5e-13),
    "dense186": (3.2e-12, 5.4e-13),
    "dense192": (4.3e-13, 5.4e-13),
    "dense198": (8.0e-13, 5.4e-13),
    "band342": (2.2e-12, 1.1e-12),
    "band180_vio": (7.0e-14, 2.3e-13),
    "band180": (7.8e-13, 8.2e-13),
    "twisted186": (1.2e-12, 5.6e-13),
    "band378": (1.3e-12, 6.0e-13),
    "bcr384": (8.7e-13, 5.9e-13),
    "bcr402": (1.1e-12, 5.6e-13),
    "bcr582": (4.8e-13, 1.1e-12),
    # the windows of the tile-kernel variants
    "w70": (1.5e-12, 9.5e-13),
    "w70_angular": (3.3e-12, 2.1e-13),
    "w70_const": (2.6e-13, 4.9e-14),
    "w70_huber": (1.8e-13, 1.1e-13),
    "g16": (9.9e-13, 5.3e-13),
    "g32": (6.6e-14, 1.9e-14),
    "g64": (7.8e-14, 2.4e-13),
    "free6": (6.1e-13, 2.9e-13),
    "lm_obs8": (1.6e-12, 4.9e-13),
    "lm_mixed": (1.7e-12, 6.2e-13),
    "lm_free1": (2.0e-12, 1.1e-12),
    "lm_free5": (2.0e-13, 6.7e-14),
}


# ---- the second step: what the candidate pass of step 1 hands to step 2 ------------------------------------------------------------------
# tests/test_gpu_second_step.py solves a window with gn_options(1) and with gn_options(2), each on a fresh handle; the second step is the
# difference of the two delta sets. The reference is the twin's own 50-digit LM loop (oracle/twin.py::lm_solve, kind="mp",
# use_schur=True) at 1 and at 2 iterations, differenced BEFORE the rounding to float64: the twin linearises by itself, so nothing of it
# passes through the oracle's Jacobians. It costs minutes, so it lives in tests/golden/second_step_ref.npz
# (tests/golden/make_golden_second_step.py).
SECOND_GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "second_step_ref.npz")
SECOND_WINDOWS = ("w70", "w70_angular")
ROW_FLOOR = 1e-11                 # the first-row tolerance of check_case
_LM1, _LM3 = {"SADVIO_LM": "1"}, {"SADVIO_LM": "1", "SADVIO_TILE_ROUNDS": "3"}
# (case, window, [(tag, switches, kernels)])
SECOND_CASES = [
    ("second_w70", "w70", [("latency", {}, "latency"), ("lm", _LM1, "throughput"), ("lm_rounds3", _LM3, "throughput")]),
    ("second_w70_angular", "w70_angular", [("latency", {}, "latency"), ("lm", _LM1, "throughput"), ("lm_rounds3", _LM3, "throughput")]),
    ("second_lm70_rounds3_subs2", "w70", [("lm_rounds3_subs2", dict(_LM3, SADVIO_LM_SUBS="2"), "throughput")]),
]


def window_case(window):
    """A case of the window (its builder and options)."""
    return next(c for c in CASES if c.window == window)


def mp_lm_state(window, iters, digits=50):
    """(x as a list of mpf, log) of the twin's 50-digit LM loop on the window after `iters` iterations."""
    from oracle import twin
    case = window_case(window)
    r = twin.lm_solve(case_window(case), case_options(case, iters), kind="mp", digits=digits, use_schur=True)
    assert r["n_success"] == iters, "the twin rejects a step"
    return list(r["x_scalar"]), np.asarray(r["log"], dtype=np.float64)


def mp_second_step(window, x1, x2, log2, digits=50):
    """The second step x2 - x1 (differenced in 50 digits, then rounded) in get_deltas layout, and row 2 of the trace."""
    import mpmath
    from oracle import twin
    mpmath.mp.dps = digits
    w = case_window(window_case(window))
    P = twin.Problem(twin.Backend("mp", digits), w)
    d = np.array([b - a for a, b in zip(x1, x2)], dtype=object)
    xp, xl = P.split(d)
    return {"pose": _to_f64(xp), "lmk": _to_f64(xl), "row": np.asarray(log2[2], dtype=np.float64)}


_refs2 = {}


def second_reference(window):
    """The 50-digit second step of the window: {"pose" [n_kf, 6], "lmk" [n_lmk, 3], "row" [8]: the trace row of step 2}."""
    if window not in _refs2:
        z = np.load(SECOND_GOLDEN)
        _refs2[window] = {k: z[f"{window}/{k}"] for k in ("pose", "lmk", "row")}
    return _refs2[window]


def second_step(d1, d2):
    """The second step of a solver from its deltas after one and after two iterations."""
    return {"pose": d2["pose"] - d1["pose"], "lmk": d2["lmk"] - d1["lmk"]}


ROW_FIELDS = ((0, "cost"), (7, "model cost change"), (2, "radius"))


def row_error(row, ref_row):
    """Largest relative distance of cost, model cost change and radius of a trace row from the reference row."""
    return max(abs(float(row[i]) / float(ref_row[i]) - 1.0) for i, _ in ROW_FIELDS)


def bars2(window):
    """(pose bar, landmark bar, row bar) of a second step."""
    e = E_REF2[window]
    return TOL_FACTOR * max(e[0], FLOOR), TOL_FACTOR * max(e[1], FLOOR), max(TOL_FACTOR * e[2], ROW_FLOOR)


# (pose part, landmark part) of step_error(the C oracle's float64 second step, 50-digit second step) and the oracle's row_error on trace
# row 2; measured by tests/test_step_reference_cpu.py::test_e_ref2_table_brackets_the_measured_values, recorded 1.5 x the measured value
E_REF2 = {
    "w70": (1.9e-12, 2.1e-12, 1.5e-13),
    "w70_angular": (2.9e-12, 8.0e-13, 1.2e-12),
}
