"""The reference of the boundary-size marginalisation tests (tests/marg_boundary.py) on the CPU: oracle.marg_information is
oracle.marginalize stopped after computeInformationAndGradient, its float64 LAPACK Schur complement and eigen-cut agree with the
full oracle at small sizes under both cuts, and every boundary case sits where its name says, unambiguously (spectral gap)."""
import numpy as np
import pytest

import marg_boundary as mb
from marg_helpers import with_lonely_landmarks
from oracle import twin
from sadvio_amd import synthetic
from sadvio_amd.synthetic import pre_marginalize
from vio_helpers import make_vio_window


def _small_case(vio):
    """A VO window (n = 3 n_keep), or the shape of test_gpu_marg.py's VIO window: IMU factor, pose priors and a previous prior."""
    if not vio:
        w = with_lonely_landmarks(synthetic.make_window(n_kf=6, n_lmk=400, seed=71, max_depth=3.0), 5, 12)
        keep, marg = pre_marginalize(w, 5)
        return w, dict(kf_marg=5, lmk_marg=marg, lmk_keep=keep[:60], priors=w.pose_priors)
    w = with_lonely_landmarks(make_vio_window(n_kf=6, n_lmk=400, seed=72, max_depth=3.0), 5, 10)
    keep, marg = pre_marginalize(w, 5)
    imu = [f for f in w.imu_factors if f["kf_i"] == 5 and f["kf_j"] == 4][0]
    rng = np.random.default_rng(7)
    prev_l = np.array(keep[:6] + marg[:2], dtype=np.int32)
    nl = 15 + 3 * len(prev_l)
    last = {"J": rng.standard_normal((nl - 3, nl)), "r0": 0.3 * rng.standard_normal(nl - 3), "kf_keep": 5, "kf_col": 0,
            "lmk_index": prev_l, "lmk_col": (15 + 3 * np.arange(len(prev_l))).astype(np.int32)}
    return w, dict(kf_marg=5, lmk_marg=marg, lmk_keep=keep[:60], kf_keep=4, marg_has_imu=True, imu=imu, priors=w.pose_priors, last=last)


@pytest.mark.parametrize("vio", [False, True])
def test_information_is_the_oracles_bit_for_bit(oracle_lib, vio):
    w, args = _small_case(vio)
    full = oracle_lib.marginalize(w, **args, want_full=True)
    info = oracle_lib.marg_information(w, **args)
    assert (info["m"], info["n"], info["kf_col"]) == (full["m"], full["n"], full["kf_col"])
    assert np.array_equal(info["lmk_col"], full["lmk_col"])
    assert np.array_equal(info["A_full"], full["A_full"]) and np.array_equal(info["b_full"], full["b_full"])
    assert np.abs(info["A_full"]).max() > 0 and np.abs(info["b_full"]).max() > 0


@pytest.mark.parametrize("eig_cut", ["reference", "noise_floor"])
@pytest.mark.parametrize("vio", [False, True])
def test_lapack_reference_matches_the_oracle(oracle_lib, vio, eig_cut):
    """twin.schur_prior (f64, np.linalg.eigh) on the oracle's A_full / b_full against oracle_marginalize's own Jacobi: the invariants
    check_prior compares (J^T J, J^T r0), bk, n_full and the layout. n <= 300; both cuts well away from every eigenvalue."""
    w, args = _small_case(vio)
    o = oracle_lib.marginalize(w, **args, eig_cut=eig_cut, want_full=True)
    m, n = o["m"], o["n"]
    assert n <= 300 and n == (15 if vio else 0) + 3 * len(args["lmk_keep"])
    t = twin.schur_prior(twin.Backend("f64"), o["A_full"], o["b_full"], m, cut=mb.CUTS[eig_cut])
    assert t["n_full"] == o["n_full"]
    Ho, Ht = o["J"].T @ o["J"], t["J"].T @ t["J"]
    scale = np.abs(Ho).max()
    assert np.abs(t["Ak"] - o["Ak"][:n, :n]).max() <= 1e-10 * np.abs(o["Ak"]).max()
    assert np.abs(Ht - Ho).max() <= 1e-10 * scale
    go = o["J"].T @ o["r0"]
    assert np.abs(t["J"].T @ t["r0"] - go).max() <= 1e-9 * max(np.abs(go).max(), np.sqrt(scale))
    assert np.abs(t["bk"] - o["bk"][:n]).max() <= 1e-9 * max(np.abs(o["bk"][:n]).max(), np.sqrt(scale))
    # the prior's range is all of Ak's here: J^T r0 = -bk (marginalization.cpp:516-530, the sign as coded)
    assert t["n_full"] == n and np.abs(go + o["bk"][:n]).max() <= 1e-8 * max(np.abs(go).max(), np.sqrt(scale))


def test_schur_prior_cut_receives_the_dimension():
    """A cut callable of (lambda_max, dim) sees m for Amm and n for Ak; one of lambda_max alone still works."""
    rng = np.random.default_rng(3)
    X = rng.standard_normal((40, 12))
    A, b = X.T @ X, rng.standard_normal(12)
    seen = []
    t = twin.schur_prior(twin.Backend("f64"), A, b, 5, cut=lambda lmax, dim: seen.append(dim) or 1e-12)
    assert seen == [5, 7] and t["n_full"] == 7
    t1 = twin.schur_prior(twin.Backend("f64"), A, b, 5, cut=lambda lmax: 1e-12)
    assert np.array_equal(t1["J"], t["J"])


def _placement(name, n, m, t):
    """Where each case must sit, in the constants of the device code."""
    chol_max = t["PCH_MAXN"] - 1   # the Cholesky form factors n + 1 columns
    if name == "vo_n1023":
        return n + 1 == t["PCH_THREADS"] and n <= t["JM_MAXN"]
    if name == "vo_n1026":
        return n > t["PCH_THREADS"] and n > t["JM_MAXN"] and n > 4 * t["JAC_THREADS"] and n - 3 < t["PCH_THREADS"]
    if name in ("vo_n2046", "vio_n2046"):
        return n <= chol_max < n + 3 and n <= t["DP_LDS_N"]
    if name in ("vo_n2049", "vio_n2049"):
        return n > t["PCH_MAXN"] and n > t["DP_LDS_N"] and n - 3 <= chol_max and n % 256 == 1
    if name == "vo_m2049":
        return m > t["PCH_MAXN"] and (m + t["WD"] - 1) // t["WD"] > 21 and n <= t["JM_MAXN"]
    raise KeyError(name)


EXPECTED = {"vo_n1023": (66, 1023), "vo_n1026": (66, 1026), "vo_n2046": (66, 2046), "vo_n2049": (66, 2049),
            "vio_n2046": (75, 2046), "vio_n2049": (75, 2049), "vo_m2049": (2049, 300)}


def test_threshold_constants_are_where_the_cases_expect():
    t = mb.thresholds()
    assert set(EXPECTED) == set(mb.CASES)
    for name, (m, n) in EXPECTED.items():
        assert _placement(name, n, m, t), (name, {k: t[k] for k in ("PCH_THREADS", "PCH_MAXN", "JM_MAXN", "JAC_THREADS", "DP_LDS_N", "WD")})


@pytest.mark.parametrize("name", sorted(mb.CASES))
def test_boundary_case_sits_on_its_threshold(oracle_lib, name):
    """Exact m and n, and a spectral gap: no eigenvalue of Amm or Ak within a factor GAP of the reference's 1e-12 or of the noise
    floor, so that both cuts keep every direction and the device's route cannot change the rank."""
    o = mb.information(name)
    assert (o["m"], o["n"]) == EXPECTED[name]
    lam_mm, lam_k = mb.spectra(name)
    for lam, dim in ((lam_mm, o["m"]), (lam_k, o["n"])):
        for cut in (1e-12, mb.noise_floor_cut(np.abs(lam).max(), dim)):
            assert np.all((lam > mb.GAP * cut) | (np.abs(lam) < cut / mb.GAP)), (name, dim, cut, lam.min())
        assert lam.min() > mb.GAP * mb.noise_floor_cut(np.abs(lam).max(), dim)    # full rank under both cuts
    for cut in ("reference", "noise_floor"):
        assert mb.reference(name, cut)["n_full"] == o["n"]
