"""CPU side of the C API's host arithmetic: the host-only headers behind the entry points as stand-alone programs. No GPU.

  tests/cpp/test_imu_host.cpp     sadvio_amd/csrc/imu_host.h: the square-root information of an IMU covariance, exp_so3 of a two-vector,
                                  the device record of a factor.
  tests/cpp/test_nofov_plan.cpp   sadvio_amd/csrc/nofov_plan.h: the fix_scale = -1 decision at its thresholds, every refusal text.
  tests/cpp/dump_nofov_tables.cpp ... its constant tables, compared here with the twin's (tests/nofov_helpers.py).
  tests/cpp/test_solve_opts.cpp   sadvio_amd/csrc/solve_opts.h: the shared option fields and the summary tail.
Each is built with -Wall -Werror and run, then built and run once more under the address and undefined-behaviour sanitizers (host code
only; nothing of it is loaded into Python or run on a GPU)."""
import os
import subprocess

import numpy as np
import pytest

import nofov_helpers as nh

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SANITIZE = ["-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-g"]
EPS = np.finfo(np.float64).eps


def _build(tmp_path, source, name, extra=()):
    exe = tmp_path / name
    subprocess.run(["g++", "-std=c++17", "-O1", "-Wall", "-Werror", *extra, os.path.join(ROOT, "tests", "cpp", source), "-o", str(exe)], check=True)
    return str(exe)


@pytest.mark.parametrize("sanitize", [False, True])
@pytest.mark.parametrize("source", ["test_imu_host.cpp", "test_nofov_plan.cpp", "test_solve_opts.cpp"])
def test_host_header(tmp_path, source, sanitize):
    r = subprocess.run([_build(tmp_path, source, source[:-4], SANITIZE if sanitize else ())], capture_output=True, text=True)
    print(r.stdout)
    assert r.returncode == 0 and r.stdout.strip().endswith("OK") and "MISMATCH" not in r.stdout, r.stdout + r.stderr


@pytest.mark.parametrize("sanitize", [False, True])
def test_nofov_tables_match_the_twin(tmp_path, sanitize):
    """3 frames, 2 cameras, cam0 = 1 (so that T_cam_cam0 is not the identity for camera 0). Every entry is at most three chained 3 x 3
    products of rotations plus a translation: 64 eps x max(1, |t|_inf)."""
    pb = dict(nh.make_nofov(seed=3, n_points=40, n_extra=2, max_lmk=4), cam0=1)
    Tf = np.asarray(pb["frame_T_f_w"], dtype=np.float64).reshape(-1, 12)
    Ts = np.asarray(pb["cam_T_s_f"], dtype=np.float64).reshape(-1, 12)
    Tm = np.asarray(pb["T_cam0_cam0p"], dtype=np.float64).reshape(12)
    assert Tf.shape[0] == 3 and Ts.shape[0] == 2
    text = f"{Tf.shape[0]} {Ts.shape[0]} {pb['cam0']}\n" + " ".join(float(x).hex() for x in np.concatenate([Tf.ravel(), Ts.ravel(), Tm]))
    r = subprocess.run([_build(tmp_path, "dump_nofov_tables.cpp", "dump_nofov_tables", SANITIZE if sanitize else ())], input=text, capture_output=True, text=True)
    assert r.returncode == 0, r.stdout + r.stderr
    rows = [ln.split() for ln in r.stdout.splitlines()]
    ftab = np.array([[float(x) for x in f[1:]] for f in rows if f[0] == "F"])
    ctab = np.array([[float(x) for x in f[1:]] for f in rows if f[0] == "C"])
    assert ftab.shape == (3, 39) and ctab.shape == (2, 15)
    # the pose table of a frame at a zero delta: R | t | Jr = I | R0 | dR = I — copies, exact
    I3 = np.eye(3).ravel()
    for k in range(3):
        assert np.array_equal(ftab[k], np.concatenate([Tf[k], I3, Tf[k][:9], I3]))
    # the scale factor's t_s = A p + b0 - lambda v with T_cam_w = T_cam_cam0 T_cam0_cam0p(lambda)^-1 T_cam0_w:
    # A = Rc R^T Rcw, b0 = Rc R^T tcw + tc, v = Rc R^T t
    T_cam0_w, T_cc0 = nh._tables(pb)
    Rcw, tcw = T_cam0_w[:9].reshape(3, 3), T_cam0_w[9:]
    R, t = Tm[:9].reshape(3, 3), Tm[9:]
    t_inf = max(np.abs(tcw).max(), np.abs(t).max(), max(np.abs(T[9:]).max() for T in T_cc0), max(np.abs(T[9:]).max() for T in Ts))
    bar = 64 * EPS * max(1.0, t_inf)
    worst = 0.0
    for c in range(2):
        Rc, tc = T_cc0[c][:9].reshape(3, 3), T_cc0[c][9:]
        B = Rc @ R.T
        want = np.concatenate([(B @ Rcw).ravel(), B @ tcw + tc, B @ t])
        worst = max(worst, np.abs(ctab[c] - want).max())
    print(f"camera tables: max |difference| {worst:.3e} (bar {bar:.3e})")
    assert worst <= bar
