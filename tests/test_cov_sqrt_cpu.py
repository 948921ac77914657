"""CPU side of the covariance's square-root assembly: the yardsticks of tests/test_gpu_cov_sqrt.py against each other, both
assemblies of the device restated in NumPy (tests/cov_sqrt_helpers.py) against them, and the host-only key-frame -> landmark lists.

E_REF of the windows with a landmark 1 mm / 0.1 mm from a camera centre, at the oracle's solution; (i) float64 Householder QR of the
whole J against the 50-digit blocks, (ii) the spread of the 50-digit blocks under one-ulp nudges of every landmark position and
key-frame translation, 8 draws. Measured (recorded, rounded up, in cov_sqrt_helpers.E_REF; DESIGN.md "Near-camera landmarks"):

    near_1e-3        (i) 9.6e-14   (ii) 2.7e-13        plain form 3.7e-4       square-root form 8.8e-15
    near_1e-4        (i) 2.4e-12   (ii) 2.8e-12        plain form indefinite   square-root form 7.0e-15
    near_1e-3_noisy  (i) 1.6e-13   (ii) 3.0e-13        plain form 3.2e-4       square-root form 5.5e-15
    band_near_1e-4   (i) 6.6e-13   (ii) 2.8e-12        plain form indefinite   square-root form 8.6e-14

The test asserts that the day's max((i), (ii)) lies in (E_REF / 4, E_REF] and that 64 x E_REF <= 1e-6.
"""
import functools
import os
import subprocess

import numpy as np
import pytest

import cov_helpers as ch
import cov_sqrt_helpers as sh
from sadvio_amd import capi, synthetic

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEAR = list(sh.WINDOWS)
FAMILIES = {   # case -> (window builder, huber_a, cross pair)
    "pixel_vo": (ch.window_pixel_vo, 0.0, (0, 1)),
    "angular_vo": (ch.window_angular_vo, 0.0, (0, 2)),
    "huber": (ch.window_huber, ch.HUBER_A, (0, 1)),
    "obs64": (ch.window_obs64, 0.0, (0, 30)),
    "lmk600": (ch.window_lmk600, 0.0, (0, 6)),
}
_oracle = {}


@pytest.fixture(scope="module", autouse=True)
def _bind_oracle(oracle_lib):
    _oracle["lib"] = oracle_lib


@functools.lru_cache(maxsize=None)
def near(case):
    """(w, oracle solution, Lin, 50-digit blocks) of a near-camera window; computed once, read only."""
    w = sh.WINDOWS[case]()
    sol = _oracle["lib"].solve(w, capi.reference_options())
    lin = sh.Lin(w, sol)
    return w, sol, lin, sh.mp_blocks_from_J(w, sol, lin=lin)


@functools.lru_cache(maxsize=None)
def family(case):
    build, huber, pair = FAMILIES[case]
    w = build()
    opts = capi.reference_options()
    opts.huber_a = huber
    sol = _oracle["lib"].solve(w, opts)
    info = ch.Information(w, sol, huber)
    return w, sol, sh.Lin(w, sol, huber), info, ch.reference_blocks(info)


@pytest.mark.parametrize("case", NEAR)
def test_yardsticks_against_each_other(case):
    w, sol, lin, mp = near(case)
    pairs = sh.PAIRS[case]
    e1 = sh.worst(sh.qr_blocks(lin), mp, lin, pairs)
    e2 = max(sh.worst(sh.mp_blocks_from_J(sh.nudged(w, 100 + t), sol), mp, lin, pairs) for t in range(8))
    e = max(e1, e2)
    print(f"[cov sqrt] {case}: e_ref (i) float64 QR of J {e1:.3e}, (ii) one-ulp nudges of the geometry {e2:.3e} (recorded {sh.E_REF[case]:.1e})")
    assert ch.TOL_FACTOR * sh.E_REF[case] <= 1e-6
    assert sh.E_REF[case] / 4 < e <= sh.E_REF[case], (case, e1, e2)
    assert mp["singular"] == []


def test_yardstick_from_J_agrees_with_the_one_from_H(oracle_lib):
    """On a window without a near-camera landmark the 50-digit blocks from J and cov_helpers.mp_blocks (50-digit inverse of the float64
    H) differ by the rounding of H alone: within that window's E_REF."""
    w, sol, lin, info, _ = family("pixel_vo")
    a = sh.mp_blocks_from_J(w, sol, lin=lin)
    b = ch.mp_blocks(info)
    e = max(sh.worst(a, dict(b, singular=info.singular), lin, [(0, 1)]), 0.0)
    print(f"[cov sqrt] pixel_vo: 50 digits from J against 50 digits from the float64 H {e:.3e}; bound {ch.E_REF['pixel_vo']:.1e}")
    assert a["singular"] == info.singular == [ch.SINGLE] and np.isnan(a["lmk"][ch.SINGLE]).all()
    assert e <= ch.E_REF["pixel_vo"]


@pytest.mark.parametrize("case", NEAR)
def test_the_bar_sees_the_plain_form_and_passes_the_square_root_form(case):
    w, sol, lin, mp = near(case)
    pairs = sh.PAIRS[case]
    tol = ch.TOL_FACTOR * sh.E_REF[case]
    pl, sq = sh.plain_form_blocks(lin), sh.sqrt_form_blocks(lin)
    e_pl = sh.worst(pl, mp, lin, pairs) if pl["usable"] else None
    e_sq = sh.worst(sq, mp, lin, pairs)
    print(f"[cov sqrt] {case}: plain form {'fails the pivot tests' if e_pl is None else format(e_pl, '.3e')}, square-root form {e_sq:.3e}; bound {tol:.3e}")
    if "1e-4" in case:
        assert not pl["usable"]
    else:
        assert e_pl >= 10 * tol
    assert sq["usable"] and e_sq <= tol
    assert pl["singular"] == sq["singular"] == mp["singular"] == []
    for l in range(w.n_lmk):
        assert np.all(np.linalg.eigvalsh(sq["lmk"][l]) >= 0.0)


@pytest.mark.parametrize("case", list(FAMILIES))
def test_square_root_form_on_the_existing_families(case):
    w, sol, lin, info, ref = family(case)
    pair = FAMILIES[case][2]
    tol = ch.TOL_FACTOR * ch.E_REF[case]
    pl, sq = sh.plain_form_blocks(lin), sh.sqrt_form_blocks(lin)
    r = dict(ref, singular=info.singular)
    e_pl, e_sq = sh.worst(pl, r, lin, [pair]), sh.worst(sq, r, lin, [pair])
    print(f"[cov sqrt] {case}: plain form {e_pl:.3e}, square-root form {e_sq:.3e}; bound {tol:.3e}")
    assert pl["usable"] and sq["usable"]
    assert pl["singular"] == sq["singular"] == info.singular
    assert e_sq <= tol and e_pl <= tol


def test_unanchored_window_fails_the_pivot_tests(oracle_lib):
    w = synthetic.make_window(n_kf=4, n_lmk=60, obs_per_lmk=4, seed=33, fixed=0)
    w.pose_priors = []
    lin = sh.Lin(w, oracle_lib.solve(w, capi.reference_options()))
    assert not sh.sqrt_form_blocks(lin)["usable"] and not sh.plain_form_blocks(lin)["usable"]


@pytest.mark.parametrize("defect", ["q_row", "list"])
def test_planted_defect_fails_the_bar(defect):
    """One row of Q1 dropped from one landmark's projection; one landmark missing from one key-frame's list."""
    case = "near_1e-3"
    w, sol, lin, mp = near(case)
    kw = dict(drop_q_row_of=17) if defect == "q_row" else dict(drop_from_list=(17, int(w.obs_kf[w.lmk_obs_ptr[17]:w.lmk_obs_ptr[18]].min())))
    if defect == "list":
        assert lin.kf_idx[kw["drop_from_list"][1]] is not None
    bad = sh.sqrt_form_blocks(lin, **kw)
    tol = ch.TOL_FACTOR * sh.E_REF[case]
    e = sh.worst(bad, mp, lin, sh.PAIRS[case]) if bad["usable"] else np.inf
    print(f"[cov sqrt] planted defect {defect}: {e:.3e}; bound {tol:.3e}")
    assert e > tol


@pytest.mark.parametrize("sanitize", [False, True])
def test_key_frame_landmark_lists(tmp_path, sanitize):
    """tests/cpp/test_cov_kf_lists.cpp, a stand-alone program over sadvio_amd/csrc/cov_kf_lists.h: plain, and under the address +
    undefined-behaviour sanitizers (host code only; nothing of it is loaded into Python or run on a GPU)."""
    exe = tmp_path / "cov_kf_lists"
    flags = ["-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-g"] if sanitize else []
    subprocess.run(["g++", "-std=c++17", "-O1", *flags, os.path.join(ROOT, "tests", "cpp", "test_cov_kf_lists.cpp"), "-o", str(exe)], check=True)
    r = subprocess.run([str(exe)], capture_output=True, text=True)
    assert r.returncode == 0 and r.stdout.strip().endswith("OK"), r.stdout + r.stderr
