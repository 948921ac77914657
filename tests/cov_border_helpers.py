"""Test infrastructure of the covariance's border route (sadvio_amd/csrc/cov_border_plan.h, cov_border_kernels.h): the windows of
tests/test_gpu_cov_border.py (cov_band_helpers' windows with a loop closure added), the planner's rule and the arrowhead recursion
restated in NumPy, the same recursion in 50 digits on top of cov_band_helpers.mp_band_inverse, and the requests the GPU tests make.
Nothing here edits cov_helpers or cov_band_helpers; the bar is their rule: a device block passes at TOL_FACTOR x E_REF of its window.

E_REF[case] is measured as cov_band_helpers says: the largest relative block difference between the float64 inverse and the 50-digit
one at the oracle's solution, over the blocks the GPU test asks for (request()); for "at_size_closure" the float64 side is the
block-sparse Schur reference with the closure factor added (schur_blocks) and the 50-digit side arrowhead_50_digits. Measured by
tests/test_cov_border_cpu.py, which asserts that the day's figure lies in (E_REF / 4, E_REF]; recorded here rounded up."""
import dataclasses

import numpy as np

import cov_band_helpers as cb
import cov_helpers as ch
from sadvio_amd import capi

COV_BORDER_MAXM = 96

E_REF = {
    "closure12": 2.3e-12,
    "closure12_hb3": 2.3e-12,
    "revisit12": 3.3e-12,
    "closure40": 6.0e-12,
    "closure_vio8": 9.5e-13,
    "closure12_angular": 5.0e-12,
    "closure12_huber": 2.5e-12,
    "at_size_closure": 1.8e-8,
}


# ---- windows --------------------------------------------------------------------------------------------------------------------
def add_relpose(w, a, b, seed=5):
    """w with one SADVIO_SPARSE_RELATIVE_POSE factor between key-frames a and b (cov_band_helpers.window_relpose's factor)."""
    from test_oracle_relative import relative_prior
    rng = np.random.default_rng(seed)
    W = np.diag(rng.uniform(20, 60, 6)) + rng.standard_normal((6, 6))
    w.sparse_priors = list(getattr(w, "sparse_priors", None) or [])
    w.sparse_priors.append(dict(type=capi.SPARSE_RELATIVE_POSE, kf=a, kf_b=b, T_prior=relative_prior(w.kf_T_f_w[a], w.kf_T_f_w[b]), sqrt_inf=W))
    return w


def window_revisit12():
    """window_vo12 and, between its landmarks, one landmark observed from the three newest and the three oldest free key-frames
    (0, 1, 2 and 8, 9, 10): nine closure edges at hb_lim = 4, which three border key-frames cover."""
    from sadvio_amd import synthetic
    a = cb.window_vo12()
    b = synthetic.make_window(n_kf=12, n_lmk=8, obs_per_lmk=22, length=6.0, seed=3)
    assert np.array_equal(a.kf_T_f_w[a.kf_const == 1], b.kf_T_f_w[b.kf_const == 1])   # same trajectory
    want = (0, 1, 2, 8, 9, 10)
    for j in range(b.n_lmk):
        k = b.obs_kf[b.lmk_obs_ptr[j]:b.lmk_obs_ptr[j + 1]]
        sel = [int(np.flatnonzero(k == q)[0]) for q in want if np.any(k == q)]
        if len(sel) == len(want):
            picks = [(a, l, None) for l in range(100)] + [(b, j, np.array(sel))] + [(a, l, None) for l in range(100, a.n_lmk)]
            return ch._assemble(a, picks)
    raise AssertionError("no landmark of the wide window is seen from both ends")


REVISIT_LMK = 100   # its index in window_revisit12()


def window_floating_half():
    """window_vo12 cut in two: only the landmarks seen from key-frames 0 .. 5 alone or from 6 .. 11 alone are kept, so the newer half
    hangs on nothing (the constant key-frame and the pose prior are in the older half), and one relative-pose factor between
    key-frames 6 and 10 closes a loop inside the older half. At hb_lim = 3 the border lies in the older half, the floating half is
    all core, and the CORE's factorisation meets the gauge freedom: a pivot of B fails its test."""
    a = cb.window_vo12()
    picks = []
    for l in range(a.n_lmk):
        k = a.obs_kf[a.lmk_obs_ptr[l]:a.lmk_obs_ptr[l + 1]]
        if k.max() <= 5 or k.min() >= 6:
            picks.append((a, l, None))
    return add_relpose(ch._assemble(a, picks), 6, 10)


def window_closure_vio8():
    """window_vio8 (dpf 15, block columns of 5) with a closure by a landmark: the library refuses a relative-pose factor on a window
    that carries IMU states, so one landmark observed from key-frames 0 and 6 (both cameras each) is appended instead. At
    hb_lim = 2 that is one closure edge and a border of one key-frame (15 columns)."""
    from sadvio_amd import synthetic
    a = cb.window_vio8()
    b = synthetic.make_window(n_kf=8, n_lmk=8, obs_per_lmk=16, length=4.0, seed=17)
    assert np.array_equal(a.kf_T_f_w[a.kf_const == 1], b.kf_T_f_w[b.kf_const == 1])   # same trajectory
    for j in range(b.n_lmk):
        o = np.arange(b.lmk_obs_ptr[j], b.lmk_obs_ptr[j + 1])
        o = o[np.isin(b.obs_kf[o], (0, 6))]
        if len(o) == 4:
            return dataclasses.replace(
                a, lmk_p=np.concatenate([a.lmk_p, b.lmk_p[[j]]]), lmk_obs_ptr=np.concatenate([a.lmk_obs_ptr, [a.n_obs + 4]]).astype(np.int32),
                obs_kf=np.concatenate([a.obs_kf, b.obs_kf[o]]).astype(np.int32), obs_cam=np.concatenate([a.obs_cam, b.obs_cam[o]]).astype(np.int32),
                obs_meas=np.concatenate([a.obs_meas, b.obs_meas[o]]), lmk_id=np.concatenate([a.lmk_id, [a.lmk_id.max() + 7]]).astype(np.int64))
    raise AssertionError("no landmark of the wide window is seen from key-frames 0 and 6 by both cameras")
AT_SIZE_CLOSURE_KF = (5, 340)


def window_at_size_closure():
    """cov_band_helpers.window_at_size (345 key-frames, N_p = 2 064) with one relative-pose factor between free key-frames 5 and
    340. The seed stays window_at_size's: the factor only adds a positive semi-definite term to an S that test_cov_band_cpu.py
    shows positive definite, and test_cov_border_cpu.py checks the sum's smallest eigenvalue again."""
    w = dataclasses.replace(cb.window_at_size())
    return add_relpose(w, *AT_SIZE_CLOSURE_KF)


WINDOWS = {   # case -> (builder, huber_a, SADVIO_COV_BORDER_HB)
    "closure12": (cb.window_relpose, 0.0, 4),
    "closure12_hb3": (cb.window_relpose, 0.0, 3),
    "revisit12": (window_revisit12, 0.0, 4),
    "closure40": (lambda: add_relpose(cb.window_vo40(), 3, 33), 0.0, 8),
    "closure_vio8": (window_closure_vio8, 0.0, 2),
    "closure12_angular": (lambda: add_relpose(cb.window_vo12(capi.FACTOR_ANGULAR), *cb.RELPOSE_KF), 0.0, 4),
    "closure12_huber": (lambda: add_relpose(cb.window_huber(), *cb.RELPOSE_KF), ch.HUBER_A, 4),
}


# ---- the planner's rule (cov_border_plan.h) ----------------------------------------------------------------------------------------
def hb_max(dpf):
    return 19 if dpf == 6 else 7


def couplings(w):
    """(cliques, pairs) in free key-frame index: per landmark its sorted distinct observing free key-frames; IMU pairs and
    relative-pose factors."""
    f = cb.free_index(w)
    cliques = []
    for l in range(w.n_lmk):
        k = f[w.obs_kf[w.lmk_obs_ptr[l]:w.lmk_obs_ptr[l + 1]]]
        k = sorted(set(int(v) for v in k if v >= 0))
        if len(k) >= 2:
            cliques.append(k)
    pairs = []
    for fac in (getattr(w, "imu_factors", None) or []):
        pairs.append((int(f[fac["kf_i"]]), int(f[fac["kf_j"]])))
    for fac in (getattr(w, "sparse_priors", None) or []):
        if fac["type"] == capi.SPARSE_RELATIVE_POSE:
            pairs.append((int(f[fac["kf"]]), int(f[fac["kf_b"]])))
    pairs = [(min(a, b), max(a, b)) for a, b in pairs if a >= 0 and b >= 0 and a != b]
    return cliques, pairs


@dataclasses.dataclass
class Plan:
    answer: str
    border: list
    core_of: list
    order: list
    hb_core: int
    n_edges: int

    @property
    def n_core(self):
        return len(self.order) - len(self.border)


def plan_rule(n_free, cliques, pairs, dpf, nb, hb_lim, fills=False):
    """The rule of cov_border_plan.h restated: closure edges, greedy vertex cover (most uncovered edges, lowest index on a tie),
    the core's hb', the answers."""
    ident = Plan("FILLED", [], list(range(n_free)), list(range(n_free)), 0, 0)
    if fills:
        return ident
    edges = set()
    for k in cliques:
        edges |= {(a, b) for i, a in enumerate(k) for b in k[i + 1:] if b - a > hb_lim}
    edges |= {(a, b) for a, b in pairs if b - a > hb_lim}
    left, border, answer = set(edges), [], "OK" if edges else "PLAIN"
    while left:
        deg = np.zeros(n_free, int)
        for a, b in left:
            deg[a] += 1; deg[b] += 1
        best = int(np.argmax(deg))          # (the first of the largest: the lowest index)
        border.append(best)
        left = {e for e in left if best not in e}
        if len(border) * dpf > COV_BORDER_MAXM:
            answer = "TOO_WIDE"
            break
    border = sorted(border)
    core_of, c = [], 0
    for k in range(n_free):
        core_of.append(-1 if k in border else c)
        c += 0 if k in border else 1
    order = [k for k in range(n_free) if k not in border] + border
    if answer == "TOO_WIDE":
        return Plan(answer, border, core_of, order, 0, len(edges))
    hb = 0
    for k in cliques:
        c = [core_of[v] for v in k if core_of[v] >= 0]
        if c:
            hb = max(hb, c[-1] - c[0])
    for a, b in pairs:
        if core_of[a] >= 0 and core_of[b] >= 0:
            hb = max(hb, core_of[b] - core_of[a])
    n_b = (n_free - len(border)) * dpf
    if answer == "OK" and (n_b % nb != 0 or n_b <= (hb + 1) * dpf):
        answer = "CORE_SHAPE"
    return Plan(answer, border, core_of, order, hb, len(edges))


def plan_of(w, hb_lim=None):
    dpf = 15 if w.has_imu else 6
    f = cb.free_index(w)
    cliques, pairs = couplings(w)
    lim = hb_max(dpf) if hb_lim is None else min(hb_lim, hb_max(dpf))
    return plan_rule(int((f >= 0).sum()), cliques, pairs, dpf, cb.block_column(dpf), lim)


def plan_input(n_free, cliques, pairs, dpf, nb, hb_lim, fills=False):
    """The input of tests/cpp/dump_cov_border_plan.cpp."""
    out = [f"{n_free} {dpf} {nb} {hb_lim} {int(fills)}", str(len(cliques))]
    out += [" ".join(str(v) for v in [len(k)] + list(k)) for k in cliques]
    out += [str(len(pairs))] + [f"{a} {b}" for a, b in pairs]
    return "\n".join(out) + "\n"


def parse_plan(text):
    rows = {ln.split()[0]: ln for ln in text.splitlines()}
    a = rows["A"].split()
    ints = lambda key: [int(v) for v in rows[key].split("|")[1].split()]
    return Plan(a[1], ints("B"), ints("C"), ints("O"), int(a[3]), int(a[2]))


# ---- the request of a GPU test ---------------------------------------------------------------------------------------------------
def request_pairs(w, plan, every=True):
    """Pairs of key-frames, by kind: inside the core band, core x border, border x border (both orders each), and one pair of core
    key-frames outside the core band in both orders. every=False: a handful of each kind (the large windows)."""
    f = cb.free_index(w)
    kf_of = {int(f[k]): k for k in range(w.n_kf) if f[k] >= 0}
    core = [k for k in range(len(plan.core_of)) if plan.core_of[k] >= 0]
    inband = [(a, b) for a in core for b in core if a != b and abs(plan.core_of[a] - plan.core_of[b]) <= plan.hb_core]
    cross = [(a, b) for a in core for b in plan.border] + [(b, a) for a in core for b in plan.border]
    bb = [(a, b) for a in plan.border for b in plan.border if a != b]
    far = [(core[0], core[-1]), (core[-1], core[0])]
    assert plan.core_of[core[-1]] - plan.core_of[core[0]] > plan.hb_core
    if not every:
        step = lambda v, n: v[::max(1, len(v) // n)][:n]
        inband, cross, bb = step(inband, 12), step(cross, 24), step(bb, 6)
    as_kf = lambda ps: [(kf_of[a], kf_of[b]) for a, b in ps]
    return {"inband": as_kf(inband), "cross": as_kf(cross), "bb": as_kf(bb), "far": as_kf(far)}


def flat_pairs(kinds):
    return kinds["inband"] + kinds["cross"] + kinds["bb"] + kinds["far"]


# ---- the arrowhead recursion in NumPy ----------------------------------------------------------------------------------------------
def column_order(plan, dpf):
    return np.concatenate([np.arange(k * dpf, (k + 1) * dpf) for k in plan.order]).astype(int)


def arrowhead_inverse(S, plan, dpf, nb, drop_zw_block=None, skip_l_row=None):
    """What the border route forms of S^-1 (natural order; NaN elsewhere): with S permuted to [B C; C^T D] by the plan,
        B = L L^T, the band of B^-1 (cov_band_helpers.band_selected_inverse), W = B^-1 C by substitution with L,
        T = D - C^T W, Sigma_DD = T^-1, Z = W T^-1, Sigma_BD = -Z, Sigma_BB = B^-1 + Z W^T inside the core band.
    Planted defects of the CPU test: drop_zw_block = (a, b), core key-frames in compacted index: that block keeps B^-1 alone;
    skip_l_row = r: the forward substitution of the first border column ignores row r of L."""
    n = S.shape[0]
    p = column_order(plan, dpf)
    nc = plan.n_core * dpf
    P = S[np.ix_(p, p)]
    B, C, D = P[:nc, :nc], P[:nc, nc:], P[nc:, nc:]
    bw = (plan.hb_core + 1) * dpf
    i, j = np.indices(B.shape)
    assert not np.any(B[np.abs(i - j) >= bw]), "the core is not banded as the plan says"
    Binv = cb.band_selected_inverse(B, bw, nb)
    L = np.linalg.cholesky(B)
    Y = np.zeros_like(C)
    for r in range(nc):
        Y[r] = (C[r] - L[r, :r] @ Y[:r]) / L[r, r]
        if skip_l_row is not None and r == skip_l_row:
            Y[r, 0] = C[r, 0] / L[r, r]
    W = np.zeros_like(C)
    for r in range(nc - 1, -1, -1):
        W[r] = (Y[r] - L[r + 1:, r] @ W[r + 1:]) / L[r, r]
    T = D - C.T @ W
    R = np.linalg.cholesky(T)
    Ri = np.linalg.inv(R)
    Tinv = Ri.T @ Ri
    Z = W @ Tinv
    ZW = Z @ W.T
    ZW = np.tril(ZW) + np.tril(ZW, -1).T
    if drop_zw_block is not None:
        a, b = drop_zw_block
        ZW[a * dpf:(a + 1) * dpf, b * dpf:(b + 1) * dpf] = 0.0
        ZW[b * dpf:(b + 1) * dpf, a * dpf:(a + 1) * dpf] = 0.0
    Xp = np.full((n, n), np.nan)
    blk = np.abs(i // dpf - j // dpf) <= plan.hb_core
    Xp[:nc, :nc] = np.where(blk, Binv + ZW, np.nan)
    Xp[:nc, nc:] = -Z
    Xp[nc:, :nc] = -Z.T
    Xp[nc:, nc:] = Tinv
    X = np.full((n, n), np.nan)
    X[np.ix_(p, p)] = Xp
    return X, dict(B=B, C=C, W=W, Z=Z, L=L, p=p, nc=nc, bw=bw)


def far_block(parts, a, b, dpf):
    """Block (a, b) of two core key-frames (compacted index, a > b) outside the core band: the column of B^-1 by substitution plus
    the Z W^T term."""
    nc, L = parts["nc"], parts["L"]
    E = np.zeros((nc, dpf)); E[b * dpf:(b + 1) * dpf] = np.eye(dpf)
    X = np.linalg.solve(L.T, np.linalg.solve(L, E))
    return X[a * dpf:(a + 1) * dpf] + parts["Z"][a * dpf:(a + 1) * dpf] @ parts["W"][b * dpf:(b + 1) * dpf].T


def reduced_blocks(w, plan, X, parts, kinds):
    """{"kf", "pair"} of the request (every key-frame; flat_pairs(kinds)) out of the arrowhead result."""
    f = cb.free_index(w)
    d = 15 if w.has_imu else 6
    kf = np.zeros((w.n_kf, d, d))
    for k in range(w.n_kf):
        if f[k] >= 0:
            kf[k] = X[f[k] * d:(f[k] + 1) * d, f[k] * d:(f[k] + 1) * d]
    pairs = flat_pairs(kinds)
    pr = np.zeros((len(pairs), d, d))
    for q, (a, b) in enumerate(pairs):
        fa, fb = int(f[a]), int(f[b])
        blk = X[fa * d:(fa + 1) * d, fb * d:(fb + 1) * d]
        if np.isnan(blk).any():
            ca, cb_ = plan.core_of[fa], plan.core_of[fb]
            assert ca >= 0 and cb_ >= 0 and abs(ca - cb_) > plan.hb_core
            blk = far_block(parts, ca, cb_, d) if ca > cb_ else far_block(parts, cb_, ca, d).T
        pr[q] = blk
    return {"kf": kf, "pair": pr}


# ---- the same recursion in 50 digits ---------------------------------------------------------------------------------------------
def dense_entries(S):
    """{(i, j): mpf} over the non-zeros of the lower triangle of the float64 matrix S."""
    import mpmath
    return {(int(i), int(j)): mpmath.mpf(float(S[i, j])) for i, j in np.argwhere(np.tril(S) != 0.0)}


def arrowhead_50_digits(S, n, plan, dpf, want, digits=50, as_float=True):
    """Entries (i, j) in `want` (natural indices) of S^-1 in 50-digit arithmetic, S given as {(i, j): mpf} over its lower triangle
    (dense_entries, SchurEntries), by the arrowhead recursion: cov_band_helpers.mp_band_inverse on the core gives the band of B^-1
    and the whole columns of B^-1 at the non-zero rows of C, from which W = B^-1 C; T, T^-1 and Z in mpmath. An entry of two core
    columns outside the core band comes from a whole column of B^-1 too."""
    import mpmath
    mpmath.mp.dps = digits
    zero = mpmath.mpf(0)
    p = column_order(plan, dpf)
    assert len(p) == n
    pos = np.empty(n, int); pos[p] = np.arange(n)
    nc, m = plan.n_core * dpf, len(plan.border) * dpf
    bw = (plan.hb_core + 1) * dpf
    Bm = cb._MpBand(nc, bw)
    C, D = {}, mpmath.matrix(m, m)
    for (i, j), v in S.items():
        a, b = int(pos[i]), int(pos[j])
        hi, lo = max(a, b), min(a, b)
        if hi < nc:
            Bm.add(hi, lo, v)
        elif lo < nc:
            C[(lo, hi - nc)] = C.get((lo, hi - nc), zero) + v
        else:
            D[hi - nc, lo - nc] += v
            if hi != lo:
                D[lo - nc, hi - nc] += v
    rows = sorted({r for r, _ in C})
    far_cols = sorted({int(min(pos[i], pos[j])) for i, j in want if pos[i] < nc and pos[j] < nc and abs(pos[i] - pos[j]) >= bw})
    band, cols = cb.mp_band_inverse(Bm, bw, sorted(set(rows) | set(far_cols)), digits)      # cols[r]: column r of B^-1, every row
    W = [[zero] * m for _ in range(nc)]
    for (r, c), v in C.items():
        col = cols[r]
        for i in range(nc):
            W[i][c] += col[i] * v
    T = D.copy()
    for (r, a), v in C.items():
        for c in range(m):
            T[a, c] -= v * W[r][c]
    Tinv = mpmath.inverse(T)
    need_rows = sorted({int(pos[i]) for i, j in want if pos[i] < nc} | {int(pos[j]) for i, j in want if pos[j] < nc})
    Zr = {r: [mpmath.fdot(W[r], (Tinv[b, c] for b in range(m))) for c in range(m)] for r in need_rows}
    out = {}
    for i, j in want:
        a, b = int(pos[i]), int(pos[j])
        if a >= nc and b >= nc:
            v = Tinv[a - nc, b - nc]
        elif a >= nc or b >= nc:
            r, c = (b, a - nc) if a >= nc else (a, b - nc)
            v = -Zr[r][c]
        else:
            hi, lo = max(a, b), min(a, b)
            base = band[(hi, lo)] if hi - lo < bw else cols[lo][hi]
            v = base + mpmath.fdot(Zr[hi], W[lo])
        out[(int(i), int(j))] = float(v) if as_float else v
    return out


def schur_entries_50_digits(sb, lmk, digits=50):
    """(S, recs): the reduced system of the SchurBlocks sb formed in 50 digits from its float64 entries of H (H_pp minus every
    landmark's H_pl H_ll^-1 H_lp, as cov_band_helpers.SchurBlocks.blocks_50_digits forms it) as {(i, j): mpf}, lower triangle; and
    per landmark of `lmk` its (H_ll^-1, H_pl H_ll^-1) in 50 digits."""
    import mpmath
    mpmath.mp.dps = digits
    mpf = mpmath.mpf
    S = dense_entries(sb.Hpp)
    recs = {}
    for l in range(sb.w.n_lmk):
        if sb.Hll[l] is None:
            continue
        Di = mpmath.inverse(mpmath.matrix([[mpf(float(v)) for v in row] for row in sb.Hll[l]]))
        Bm = mpmath.matrix([[mpf(float(v)) for v in row] for row in sb.Hpl[l]])
        BD = Bm * Di
        upd = BD * Bm.T
        rows = [int(r) for r in sb.rows[l]]
        for a, ra in enumerate(rows):
            for b, rb in enumerate(rows):
                if ra >= rb:
                    S[(ra, rb)] = S.get((ra, rb), mpf(0)) - upd[a, b]
        if l in lmk:
            recs[l] = (Di, BD)
    return S, recs


# ---- block-sparse Schur reference of the at-size closure window ---------------------------------------------------------------------
def schur_blocks(w, deltas):
    """cov_band_helpers.SchurBlocks of w without its relative-pose factors (SchurBlocks carries landmarks and pose priors only), the
    factors' own information then added to H_pp: the difference of cov_helpers.Information on a one-landmark sub-window with and
    without them, so every float64 entry is still one Information forms."""
    bare = dataclasses.replace(w)
    bare.sparse_priors = []
    sb = cb.SchurBlocks(bare, deltas)
    sub0 = ch._assemble(bare, [(bare, 0, None)])
    sub1 = ch._assemble(bare, [(bare, 0, None)])
    sub1.sparse_priors = list(w.sparse_priors)
    d = {"pose": deltas["pose"], "lmk": deltas["lmk"][[0]]}
    i0, i1 = ch.Information(sub0, d), ch.Information(sub1, d)
    pidx = np.concatenate([idx for idx in i0.kf_idx if idx is not None])
    sb.Hpp += i1.H[np.ix_(pidx, pidx)] - i0.H[np.ix_(pidx, pidx)]
    sb.w = w
    return sb
