"""GPU parity of sadvio_ba_marginalize on both sides of every size threshold of its routes (marg_driver.h: run_pchol, run_jacobi_rows,
run_jacobi, the Amm route, the Cholesky form's limit), against the float64 LAPACK reference of tests/marg_boundary.py. The route a
call took is invisible in its result; it is read from the sweep counts, marg_stats and the SADVIO_DEBUG=16384 lines ("block jacobi
n ..." for the Cholesky-preconditioned block Jacobi, "jacobi n ..." for the plain one), which the handle reads once at creation."""
import re

import numpy as np
import pytest

import marg_boundary as mb
from sadvio_amd import capi

pytestmark = pytest.mark.gpu


def _marginalize(backend_cls, monkeypatch, name, eig_cut, form):
    monkeypatch.setenv("SADVIO_DEBUG", "16384")
    w, args = mb.case(name)
    be = backend_cls(device=0)
    try:
        be.set_windows([w])
        g = be.marginalize(0, **args, eig_cut=eig_cut, form=form)
        stats = be.marg_stats()
    finally:
        be.close()
    return g, stats


def _plain_jacobi_converged(err, n):
    """The plain Jacobi ran on an n x n matrix and ended on a sweep without rotations, inside its 40-sweep cap."""
    sweeps = [int(r) for r in re.findall(rf"\] jacobi n {n} sweep \d+ rotations (\d+)", err)]
    return len(sweeps) > 0 and sweeps[-1] == 0 and len(sweeps) < 40


@pytest.mark.parametrize("form", ["eigen", "cholesky"])
@pytest.mark.parametrize("name", ["vo_n1023", "vo_n1026"])
def test_prior_across_pch_threads(backend_cls, monkeypatch, capfd, name, form):
    """n = 1 023 / 1 026 around PCH_THREADS = JM_MAXN = 1 024. Eigen form: pivoted Cholesky k_pchol_panel_rx<1,32> / <2,16> (each thread
    owns i and i + 1 024), block Jacobi k_jacobi_mma / k_jacobi_block<8>. Cholesky form: n + 1 = 1 024 / 1 027 columns."""
    g, _ = _marginalize(backend_cls, monkeypatch, name, "noise_floor", form)
    err = capfd.readouterr().err
    n = g["n"]
    assert g["sweeps"][0] == 0                                  # Amm (m = 66) by its Cholesky factor
    if form == "eigen":
        assert f"relaxed pivoted cholesky n {n} " in err and f"block jacobi n {n} " in err and f"] jacobi n {n} " not in err
    else:
        assert f"relaxed pivoted cholesky n {n + 1} " in err and "block jacobi" not in err and g["sweeps"] == (0, 0)
    mb.check_prior(g, mb.reference(name, "noise_floor"), orthogonal=form == "eigen")


def test_cholesky_form_at_its_largest_size_pivoted(backend_cls, monkeypatch, capfd):
    """n = 2 046, n + 1 = 2 047 <= PCH_MAXN: the largest Cholesky-form prior, rank-revealing pivoted route (noise floor)."""
    g, stats = _marginalize(backend_cls, monkeypatch, "vo_n2046", "noise_floor", "cholesky")
    err = capfd.readouterr().err
    assert "relaxed pivoted cholesky n 2047 " in err and stats == {"calls": 1, "unpivoted": 0, "fell_back": 0}
    mb.check_prior(g, mb.reference("vo_n2046", "noise_floor"), orthogonal=False)


def test_cholesky_form_at_its_largest_size_unpivoted(backend_cls, monkeypatch, capfd):
    """n = 15 + 2 031 = 2 046 (VIO: kf_keep, IMU factor, a full-rank previous prior with nl = 81 >= 64): under the reference's cut
    behind a full-rank previous prior the factor is the unpivoted wide-panel one (run_wfac, 22 panels)."""
    g, stats = _marginalize(backend_cls, monkeypatch, "vio_n2046", "reference", "cholesky")
    err = capfd.readouterr().err
    assert stats == {"calls": 1, "unpivoted": 1, "fell_back": 0} and "relaxed pivoted cholesky n 2047 " not in err
    assert g["sweeps"] == (0, 0) and g["kf_col"] == 0
    mb.check_prior(g, mb.reference("vio_n2046", "reference"), orthogonal=False)


def test_eigen_form_at_pch_maxn(backend_cls, monkeypatch, capfd):
    """n = 2 046 <= PCH_MAXN: the eigen form still takes the Cholesky-preconditioned block Jacobi (k_jacobi_block<8>)."""
    g, _ = _marginalize(backend_cls, monkeypatch, "vo_n2046", "noise_floor", "eigen")
    err = capfd.readouterr().err
    assert "relaxed pivoted cholesky n 2046 " in err and "block jacobi n 2046 " in err and "] jacobi n 2046 " not in err
    mb.check_prior(g, mb.reference("vo_n2046", "noise_floor"))


@pytest.mark.parametrize("eig_cut", ["noise_floor", "reference"])
def test_eigen_form_past_pch_maxn(backend_cls, monkeypatch, capfd, eig_cut):
    """n = 2 049 > PCH_MAXN: Ak through the plain one-sided Jacobi (k_jacobi_step), which must converge inside its sweep cap."""
    g, _ = _marginalize(backend_cls, monkeypatch, "vo_n2049", eig_cut, "eigen")
    err = capfd.readouterr().err
    assert _plain_jacobi_converged(err, 2049) and "block jacobi n 2049 " not in err and 0 < g["sweeps"][1] <= 40
    mb.check_prior(g, mb.reference("vo_n2049", eig_cut))


def test_vio_eigen_form_past_pch_maxn(backend_cls, monkeypatch, capfd):
    """n = 15 + 2 034 = 2 049 (VIO, IMU factor, previous prior with nl = 81 >= 64) under the reference's cut: plain Jacobi on Ak."""
    g, _ = _marginalize(backend_cls, monkeypatch, "vio_n2049", "reference", "eigen")
    err = capfd.readouterr().err
    assert _plain_jacobi_converged(err, 2049) and g["kf_col"] == 0
    mb.check_prior(g, mb.reference("vio_n2049", "reference"))


def test_cholesky_form_refused_past_pch_maxn(backend_cls):
    """n = 2 049: n + 1 > PCH_MAXN, the Cholesky form is refused with SADVIO_E_INVALID_ARG; the handle still marginalises."""
    w, args = mb.case("vo_n2049")
    be = backend_cls(device=0)
    try:
        be.set_windows([w])
        with pytest.raises(capi.SadvioError) as ei:
            be.marginalize(0, **args, form="cholesky")
        assert f"rc={capi.E_INVALID_ARG}:" in str(ei.value) and "the Cholesky form handles n < 2048" in str(ei.value)
        g = be.marginalize(0, **args, form="eigen")
    finally:
        be.close()
    mb.check_prior(g, mb.reference("vo_n2049", "noise_floor"))


def test_amm_past_pch_maxn_noise_floor(backend_cls, monkeypatch, capfd):
    """m = 6 + 2 043 = 2 049 > PCH_MAXN under the noise floor: Amm takes the plain Jacobi (no Cholesky route is tried)."""
    g, _ = _marginalize(backend_cls, monkeypatch, "vo_m2049", "noise_floor", "eigen")
    err = capfd.readouterr().err
    assert _plain_jacobi_converged(err, 2049) and g["sweeps"][0] > 0 and "block jacobi n 300 " in err
    mb.check_prior(g, mb.reference("vo_m2049", "noise_floor"))


def test_amm_past_pch_maxn_reference_cut(backend_cls, monkeypatch, capfd):
    """m = 2 049 under the reference's cut: Amm by the unpivoted wide-panel factor (run_wfac, 22 panels of 96), no Jacobi on Amm."""
    g, _ = _marginalize(backend_cls, monkeypatch, "vo_m2049", "reference", "eigen")
    err = capfd.readouterr().err
    assert g["sweeps"][0] == 0 and "jacobi n 2049 " not in err and "relaxed pivoted cholesky n 2049 " not in err
    mb.check_prior(g, mb.reference("vo_m2049", "reference"))
