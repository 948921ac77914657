"""CPU side of sadvio_ba_covariance_cross: the float64 yardsticks of tests/test_gpu_cov_cross.py, the device formula of both
assemblies restated in NumPy, planted defects that the bar must see, the ctypes mirror of sadvio_cov_cross_request and the stand-alone
program over cov_cross_plan.h. No GPU.

E_REF_CROSS / E_REF_INNOV per case = the worst cross norm / innovation figure (cov_cross_helpers) of np.linalg.inv of the full
information matrix against its 50-digit inverse over the case's candidates, at the oracle's solution. Measured values (recorded,
rounded up, in cov_cross_helpers):

                 cross      innovation                            cross      innovation
    pixel_vo     2.29e-12   3.64e-12  (n = 129)      obs64        5.28e-13   1.15e-12  (n = 789)
    angular_vo   3.70e-13   3.55e-11  (n = 138)      lmk600       4.56e-13   9.10e-13  (n = 1857)
    huber        2.40e-12   1.67e-11  (n = 129)      vo12         1.32e-12   9.81e-12  (n = 666)
    vio_dense    1.24e-09   1.52e-07  (n = 420)      vio8         2.20e-13   8.09e-13  (n = 585)
    near_1e-3    1.07e-08   (2.5e-2: no yardstick, see cov_cross_helpers)
    near_1e-4    1.91e-07   (2.0e+2: none)             at_size      5.80e-08   1.22e-07  (N_p = 2064, bw = 36)

Every yardstick test asserts that the day's figure lies in (E / 4, E]."""
import ctypes as C
import functools
import os
import re
import subprocess

import numpy as np
import pytest

import cov_band_helpers as bh
import cov_cross_helpers as xh
import cov_helpers as ch
import cov_sqrt_helpers as sh
from sadvio_amd import capi

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@functools.lru_cache(maxsize=None)
def _case(case):
    from oracle import oracle
    oracle.build()
    build, huber, cands = xh.CASES[case]
    if build is None:
        from test_cov_cpu import _vio_windows
        w = _vio_windows(oracle)[0]
    else:
        w = build()
    opts = capi.reference_options()
    opts.huber_a = huber
    sol = oracle.solve(w, opts, dense_prior=getattr(w, "dense_prior", None))
    info = ch.Information(w, sol, huber)
    kf, lmk = cands(w)
    cam, meas = xh.candidate_observations(w, sol, kf, lmk)
    return w, sol, huber, info, np.linalg.inv(info.H), kf, lmk, cam, meas


@functools.lru_cache(maxsize=None)
def _mp(case):
    _, _, _, info, _, _, lmk, _, _ = _case(case)
    return xh.mp_inverse_for(info, lmk)


@pytest.mark.parametrize("case", list(xh.CASES))
def test_float64_against_50_digits(case):
    w, sol, _, info, X, kf, lmk, cam, meas = _case(case)
    X50 = _mp(case)
    f64 = xh.reference_result(w, info, X, sol, kf, lmk, cam, meas)
    e_cross, e_innov = xh.worst_errors(w, info, X50, sol, kf, lmk, cam, meas, f64)
    n_inv = int((f64["status"] == xh.CROSS_PROJ_INVALID).sum())
    print(f"[cov cross] {case}: n {info.n}, {len(kf)} candidates ({n_inv} with an invalid projection), e_ref cross {e_cross:.3e} "
          f"(recorded {xh.E_REF_CROSS[case]:.1e}), innovation {e_innov:.3e} (recorded {xh.E_REF_INNOV.get(case, float('nan')):.1e})")
    assert xh.E_REF_CROSS[case] / 4 < e_cross <= xh.E_REF_CROSS[case], (case, e_cross)
    if case in xh.E_REF_INNOV:
        assert xh.E_REF_INNOV[case] / 4 < e_innov <= xh.E_REF_INNOV[case], (case, e_innov)


def _device_formula(lin, blocks_fn, sqrt, skip_entry=None, untransposed=False):
    """Sigma_al of every (free key-frame, eliminated landmark) by the device formula from the assembly restated in NumPy
    (cov_sqrt_helpers): plain -Sigma_pp W^T, square-root -Sigma_pp C^T R^-T. Planted defects: skip_entry = l: the first observing
    key-frame of landmark l is left out of its sum; untransposed: W_e used as stored (3 x 6 read as 6 x 3)."""
    J, p = lin.J, lin.p
    out = blocks_fn(lin)
    assert out["usable"]
    sub = [None if idx is None else np.array([lin.pos[int(c)] for c in idx]) for idx in lin.kf_idx]
    Spp = np.zeros((len(p), len(p)))
    for a, sa in enumerate(sub):
        for b, sb in enumerate(sub):
            if sa is not None and sb is not None:
                Spp[np.ix_(sa, sb)] = out["cross"](a, b) if a != b else out["kf"][a]
    res = {}
    for l, idx in enumerate(lin.lmk_idx):
        if idx is None or l in out["singular"]:
            continue
        rows = lin.lmk_rows[l]
        Jl, Jp = J[np.ix_(rows, idx)], J[np.ix_(rows, p)]
        if sqrt:
            Q, R = sh.gram_schmidt_2(Jl)
            Wl = Q.T @ Jp                                      # C
        else:
            Wl = sh._sym3_inverse(Jl.T @ Jl) @ (Jl.T @ Jp)     # W
        ents = [k for k, s in enumerate(sub) if s is not None and np.any(Wl[:, s[:6]] != 0.0)]
        for a, sa in enumerate(sub):
            if sa is None:
                continue
            acc = np.zeros((len(sa), 3))
            for q, k in enumerate(ents):
                if skip_entry == l and q == 0:
                    continue
                We = Wl[:, sub[k][:6]]                         # 3 x 6
                Sg = Spp[np.ix_(sa, sub[k][:6])]
                acc += Sg @ (We.reshape(6, 3) if untransposed else We.T)
            res[(a, l)] = -(acc @ np.linalg.inv(R).T) if sqrt else -acc
    return res


@pytest.mark.parametrize("case,sqrt", [("pixel_vo", False), ("pixel_vo", True), ("near_1e-3", True), ("angular_vo", False)])
def test_device_formula_in_numpy(case, sqrt):
    w, sol, huber, info, X, kf, lmk, _, _ = _case(case)
    lin = sh.Lin(w, sol, huber)
    got = _device_formula(lin, sh.sqrt_form_blocks if sqrt else sh.plain_form_blocks, sqrt)
    e = max(xh.cross_error(got[(int(k), int(l))], info, X, int(k), int(l)) for k, l in zip(kf, lmk) if (int(k), int(l)) in got)
    tol = ch.TOL_FACTOR * xh.E_REF_CROSS[case]
    print(f"[cov cross] {case} {'square-root' if sqrt else 'plain'} formula against the full inverse: {e:.3e}; bound {tol:.3e}")
    assert e <= tol


@pytest.mark.parametrize("defect", ["observer", "untransposed"])
def test_planted_defects_are_caught(defect):
    case = "pixel_vo"
    w, sol, huber, info, X, kf, lmk, _, _ = _case(case)
    lin = sh.Lin(w, sol, huber)
    l_bad = 12
    got = _device_formula(lin, sh.plain_form_blocks, False, skip_entry=l_bad if defect == "observer" else None, untransposed=defect == "untransposed")
    e = max(xh.cross_error(got[(k, l_bad)], info, X, k, l_bad) for k in range(w.n_kf) if (k, l_bad) in got)
    tol = ch.TOL_FACTOR * xh.E_REF_CROSS[case]
    print(f"[cov cross] planted defect {defect}: {e:.3e}; bound {tol:.3e}")
    assert e > tol


@pytest.mark.parametrize("case", ["vo12", "vio8"])
def test_band_row_stopped_at_the_band_edge_is_caught(case):
    """k_cov_band_cols gives Sigma[i][col] only for rows i >= col + d. A block row taken from it (zeros above the key-frame's own
    block) misses the bar on the candidates whose observers lie above the band's edge."""
    w, sol, huber, info, X, kf, lmk, _, _ = _case(case)
    S, cols = bh.schur(info)
    Spp = np.linalg.inv(S)
    f = bh.free_index(w)
    worst = 0.0
    for k, l in zip(kf, lmk):
        k, l = int(k), int(l)
        if cols[k] < 0 or info.lmk_idx[l] is None or l in info.singular:
            continue
        ia, il = info.kf_idx[k], info.lmk_idx[l]
        pidx = np.concatenate([idx for idx in info.kf_idx if idx is not None])
        Wl = np.linalg.solve(info.H[np.ix_(il, il)], info.H[np.ix_(il, pidx)])     # 3 x N_p
        row = Spp[cols[k]:cols[k] + info.d].copy()
        good = -row @ Wl.T
        assert xh.cross_error(good, info, X, k, l) <= ch.TOL_FACTOR * xh.E_REF_CROSS[case]
        row[:, :cols[k]] = 0.0                                                     # the substitution stopped at the band's edge
        worst = max(worst, xh.cross_error(-row @ Wl.T, info, X, k, l))
    tol = ch.TOL_FACTOR * xh.E_REF_CROSS[case]
    print(f"[cov cross] {case}: band row stopped at the edge: {worst:.3e}; bound {tol:.3e}")
    assert worst > tol and f.max() > 0


@pytest.mark.parametrize("case", [c for c in xh.E_REF_INNOV if c in xh.CASES])
def test_innovation_without_the_cross_block_misses_the_bar(case):
    """On every test window P with Sigma_al dropped differs from the true P by more than the bar: the GPU test tells the feature
    from its absence."""
    w, sol, _, info, X, kf, lmk, cam, meas = _case(case)
    bad = xh.reference_result(w, info, X, sol, kf, lmk, cam, meas, drop_cross=True)
    ref = xh.reference_result(w, info, X, sol, kf, lmk, cam, meas)
    e = max(ch.rel_diff(bad["innov"][i], ref["innov"][i]) for i in range(len(kf)) if ref["status"][i] != xh.CROSS_LMK_SINGULAR)
    tol = ch.TOL_FACTOR * xh.E_REF_INNOV[case]
    print(f"[cov cross] {case}: P without Sigma_al differs by {e:.3e}; bound {tol:.3e}")
    assert e > tol


def test_cross_request_mirror_matches_the_c_header(tmp_path):
    hdr = open(os.path.join(ROOT, "include", "sadvio_ba.h")).read()
    hdr = re.sub(r"/\*.*?\*/", "", hdr, flags=re.S)
    m = re.search(r"typedef struct sadvio_cov_cross_request\s*\{(.*?)\}\s*sadvio_cov_cross_request;", hdr, flags=re.S)
    assert m
    fields = [d.strip().split()[-1].lstrip("*") for d in m.group(1).split(";") if d.strip()]
    assert fields == [f for f, _ in capi.CovCrossRequestC._fields_]
    lines = ['#include <cstdio>', '#include <cstddef>', '#include "sadvio_ba.h"', "int main() {",
             'std::printf("sizeof %zu\\n", sizeof(sadvio_cov_cross_request));']
    lines += [f'std::printf("{f} %zu\\n", offsetof(sadvio_cov_cross_request, {f}));' for f in fields]
    lines += ['std::printf("codes %d %d %d\\n", SADVIO_CROSS_OK, SADVIO_CROSS_LMK_SINGULAR, SADVIO_CROSS_PROJ_INVALID);', "return 0; }"]
    src = tmp_path / "layout.cpp"
    src.write_text("\n".join(lines))
    exe = tmp_path / "layout"
    subprocess.run(["g++", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe)], check=True)
    out = subprocess.run([str(exe)], check=True, capture_output=True, text=True).stdout.splitlines()
    lay = dict(ln.split(None, 1) for ln in out)
    assert int(lay["sizeof"]) == C.sizeof(capi.CovCrossRequestC)
    for f in fields:
        assert int(lay[f]) == getattr(capi.CovCrossRequestC, f).offset, f
    assert lay["codes"].split() == [str(capi.CROSS_OK), str(capi.CROSS_LMK_SINGULAR), str(capi.CROSS_PROJ_INVALID)]
    decl = re.search(r"int sadvio_ba_covariance_cross\((.*?)\);", hdr, flags=re.S).group(1)
    assert len(decl.split(",")) == 7


@pytest.mark.parametrize("sanitize", [False, True])
def test_cross_plan(tmp_path, sanitize):
    """tests/cpp/test_cov_cross_plan.cpp, a stand-alone program over sadvio_amd/csrc/cov_cross_plan.h: plain, and under the address +
    undefined-behaviour sanitizers (host code only; nothing of it is loaded into Python or run on a GPU)."""
    exe = tmp_path / "cov_cross_plan"
    flags = ["-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-g"] if sanitize else []
    subprocess.run(["g++", "-std=c++17", "-O1", *flags, os.path.join(ROOT, "tests", "cpp", "test_cov_cross_plan.cpp"), "-o", str(exe)], check=True)
    r = subprocess.run([str(exe)], capture_output=True, text=True)
    assert r.returncode == 0 and r.stdout.strip().endswith("OK"), r.stdout + r.stderr


def test_float64_against_50_digits_at_size():
    """The 345-key-frame window (N_p = 2 064; the full matrix has 11 379 columns): the float64 side is the block-sparse Schur reference
    (cov_band_helpers.SchurBlocks: np.linalg.inv of S), the 50-digit side the band Cholesky factor, the Takahashi recursion and whole
    columns by band substitution in mpmath on the same float64 entries, for the three key-frames x 20 landmarks the GPU test asks."""
    from oracle import oracle
    oracle.build()
    w = bh.window_at_size()
    sol = oracle.solve(w, capi.reference_options())
    hb, bw, _ = bh.bandwidth(w)
    kf, lmk = xh.at_size_candidates(w)
    cam, meas = xh.candidate_observations(w, sol, kf, lmk)
    sb = bh.SchurBlocks(w, sol)
    info, X = xh.at_size_reference(sb, bw, kf, lmk)
    info50, X50 = xh.at_size_reference(sb, bw, kf, lmk, digits=50)
    f64 = xh.reference_result(w, info, X, sol, kf, lmk, cam, meas)
    e_cross, e_innov = xh.worst_errors(w, info50, X50, sol, kf, lmk, cam, meas, f64)
    print(f"[cov cross] at_size: N_p {sb.n}, bw {bw}, {len(kf)} candidates, e_ref cross {e_cross:.3e} (recorded {xh.E_REF_CROSS['at_size']:.1e}), "
          f"innovation {e_innov:.3e} (recorded {xh.E_REF_INNOV['at_size']:.1e})")
    assert xh.E_REF_CROSS["at_size"] / 4 < e_cross <= xh.E_REF_CROSS["at_size"], e_cross
    assert xh.E_REF_INNOV["at_size"] / 4 < e_innov <= xh.E_REF_INNOV["at_size"], e_innov
