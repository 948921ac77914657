"""Marginalisation windows sized to sit on the route thresholds of sadvio_ba_marginalize (marg_driver.h: run_pchol, run_jacobi_rows,
run_jacobi, the Amm route) and of the dense prior kernels (kernels.h: k_prior_r / k_prior_m), and the float64 LAPACK reference of
their prior: the oracle's A = sum J^T J, b = sum J^T r (oracle.marg_information, computeInformationAndGradient), then the Schur
complement and the eigen-cut of marginalization.cpp:213-265,318-342,516-530 with np.linalg.eigh (twin.schur_prior, f64). The oracle's
own cyclic Jacobi takes minutes at these sizes; tests/test_marg_boundary_cpu.py pins this reference against it at small ones.

Every case is built so that no eigenvalue of Amm or Ak lies within a factor GAP of either cut: the result must not depend on which
side of a cut a near-null eigenvalue falls (near landmarks, the best-observed candidates first, frame0 carries its pose prior)."""
import functools
import os
import re

import numpy as np

from marg_helpers import with_lonely_landmarks
from sadvio_amd import synthetic
from sadvio_amd.synthetic import pre_marginalize

CSRC = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "sadvio_amd", "csrc")
EPS = 2.220446049250313e-16
GAP = 1e3


def thresholds():
    """The route constants as the device code defines them (constexpr int A = 1[, B = 2 ...]; in the csrc headers)."""
    out = {}
    for f in sorted(os.listdir(CSRC)):
        if f.endswith(".h"):
            with open(os.path.join(CSRC, f)) as fh:
                for decl in re.findall(r"constexpr int ([^;]+);", fh.read()):
                    for name, val in re.findall(r"(\w+) = (\d+)\s*(?:,|$)", decl):
                        out[name] = int(val)
    return out


def noise_floor_cut(lmax, dim):
    """SADVIO_EIG_CUT_NOISE_FLOOR (oracle/marg.c: marg_cut): the reference's 1e-12 with the floor dim * eps * lambda_max."""
    return max(1e-12, dim * EPS * lmax)


CUTS = {"reference": 1e-12, "noise_floor": noise_floor_cut}


@functools.lru_cache(maxsize=None)
def _window(kind, seed, n_lonely):
    """A 6-key-frame window with landmarks at 1 .. 3 m (the depth of far ones is too weakly observed for the gap), n_lonely of frame0's
    landmarks made lonely; the keep / marg candidates of preMarginalize, each ordered best-observed first."""
    if kind == "vo":
        w = synthetic.make_window(n_kf=6, n_lmk=8000, seed=seed, max_depth=3.0)
    else:
        from vio_helpers import make_vio_window
        w = make_vio_window(n_kf=6, n_lmk=8000, seed=seed, max_depth=3.0)
    kf0 = w.n_kf - 1
    w = with_lonely_landmarks(w, kf0, n_lonely)
    keep, marg = pre_marginalize(w, kf0)
    return w, kf0, _best_observed(w, kf0, keep), _best_observed(w, kf0, marg)


def _best_observed(w, kf0, lmks):
    """Landmarks ordered by the smallest eigenvalue of the 3 x 3 information block frame0 gives them, largest first."""
    from oracle import oracle
    A = oracle.marg_information(w, kf0, [], lmks)["A_full"]
    lam = [np.linalg.eigvalsh(A[6 + 3 * k:9 + 3 * k, 6 + 3 * k:9 + 3 * k])[0] for k in range(len(lmks))]
    return [lmks[k] for k in np.argsort(lam, kind="stable")[::-1]]


# name -> (kind, n_keep, n_marg): n = (15 if VIO) + 3 n_keep, m = (15 if VIO else 6) + 3 n_marg
CASES = {
    "vo_n1023": ("vo", 341, 20),     # n = 1 023 = PCH_THREADS - 1: Cholesky form n + 1 = PCH_THREADS; k_jacobi_mma at n <= JM_MAXN
    "vo_n1026": ("vo", 342, 20),     # n = 1 026 > PCH_THREADS, JM_MAXN: k_pchol_panel_rx<2,16>, k_jacobi_block<8>
    "vo_n2046": ("vo", 682, 20),     # n = 2 046: Cholesky form n + 1 = 2 047 <= PCH_MAXN (the largest); eigen form pchol + block Jacobi
    "vo_n2049": ("vo", 683, 20),     # n = 2 049 > PCH_MAXN, DP_LDS_N: plain Jacobi on Ak; the Cholesky form is refused
    "vio_n2046": ("vio", 677, 20),   # n = 15 + 2 031 = 2 046: Cholesky form, unpivoted route behind a full-rank previous prior
    "vio_n2049": ("vio", 678, 20),   # n = 15 + 2 034 = 2 049: eigen form through the plain Jacobi, IMU + previous prior
    "vo_m2049": ("vo", 100, 681),    # m = 6 + 2 043 = 2 049 > PCH_MAXN: Amm through the plain Jacobi / run_wfac with 22 panels
}
SEEDS = {"vo": 91, "vio": 92}
N_LONELY = {"vo_m2049": 1500}


def case(name):
    """(window, marginalize() arguments) of a named case; `last` (VIO) is a full-rank previous prior over frame0's 15 states and 22
    landmarks (nl = 81 >= 64: the H = J^T J scatter of a caller-supplied prior)."""
    kind, n_keep, n_marg = CASES[name]
    w, kf0, keep, marg = _window(kind, SEEDS[kind], N_LONELY.get(name, 60))
    if kind == "vo":
        args = dict(kf_marg=kf0, lmk_marg=marg[:n_marg], lmk_keep=keep[:n_keep], priors=w.pose_priors)
    else:
        kf1 = kf0 - 1
        imu = [f for f in w.imu_factors if f["kf_i"] == kf0 and f["kf_j"] == kf1][0]
        rng = np.random.default_rng(5)
        prev_l = np.array(keep[:20] + marg[:2], dtype=np.int32)
        nl = 15 + 3 * len(prev_l)
        last = {"J": 20.0 * (np.eye(nl) + 0.1 * rng.standard_normal((nl, nl))), "r0": 0.1 * rng.standard_normal(nl), "kf_keep": kf0,
                "kf_col": 0, "lmk_index": prev_l, "lmk_col": (15 + 3 * np.arange(len(prev_l))).astype(np.int32)}
        args = dict(kf_marg=kf0, lmk_marg=marg[:n_marg], lmk_keep=keep[:n_keep], kf_keep=kf1, marg_has_imu=True, imu=imu,
                    priors=w.pose_priors, last=last)
    assert len(args["lmk_keep"]) == n_keep and len(args["lmk_marg"]) == n_marg
    return w, args


@functools.lru_cache(maxsize=None)
def information(name):
    from oracle import oracle
    w, args = case(name)
    return oracle.marg_information(w, **args)


@functools.lru_cache(maxsize=None)
def reference(name, eig_cut):
    """The prior of case `name` under `eig_cut` in float64 LAPACK, with the keys check_prior reads."""
    from oracle import twin
    o = information(name)
    t = twin.schur_prior(twin.Backend("f64"), o["A_full"], o["b_full"], o["m"], cut=CUTS[eig_cut])
    return {"J": t["J"], "r0": t["r0"], "Ak": t["Ak"], "bk": t["bk"], "n_full": t["n_full"], "m": o["m"], "n": o["n"],
            "kf_col": o["kf_col"], "lmk_col": o["lmk_col"]}


def spectra(name):
    """Eigenvalues of Amm (symmetrised, as decomposed) and of the noise-floor reference's Ak."""
    o, m = information(name), information(name)["m"]
    A = o["A_full"]
    Ak = reference(name, "noise_floor")["Ak"]
    return np.linalg.eigvalsh((A[:m, :m] + A[:m, :m].T) / 2), np.linalg.eigvalsh((Ak + Ak.T) / 2)


def check_prior(g, o, rtol=1e-8, orthogonal=True):
    """The prior's invariants (tests/test_gpu_marg.py: check_prior), row orthogonality for the eigen form only."""
    assert g is not None and o is not None
    assert (g["m"], g["n"], g["n_full"], g["kf_col"]) == (o["m"], o["n"], o["n_full"], o["kf_col"])
    assert np.array_equal(g["lmk_col"], o["lmk_col"])
    Hg, Ho = g["J"].T @ g["J"], o["J"].T @ o["J"]
    scale = np.abs(Ho).max()
    assert np.abs(Hg - Ho).max() <= rtol * scale
    gg, go = g["J"].T @ g["r0"], o["J"].T @ o["r0"]
    assert np.abs(gg - go).max() <= rtol * max(np.abs(go).max(), np.sqrt(scale))
    if orthogonal:
        JJ = g["J"] @ g["J"].T
        assert np.abs(JJ - np.diag(np.diag(JJ))).max() <= 1e-8 * scale
