#!/usr/bin/env python
"""Time of one sadvio_ba_covariance_cross call against sadvio_ba_covariance on the same build and handle.

  python scripts/gpu_time_covariance_cross.py [CALLS] [OUT]      # OUT: default profiles/r20_covariance_cross_time.txt

The request: the newest key-frame x every landmark of the window, with a candidate observation each (camera 0, the predicted
measurement + 3 px), so that cross blocks, innovation covariances and maha2 are all formed. Windows: the shipped VIO window (12 KF
with IMU states, ~2 900 landmarks), config 2 (20 KF x 8 000 landmarks) and the 345-key-frame window of tests/cov_band_helpers.py
(N_p = 2 064: the band route). Baseline: sadvio_ba_covariance for all key-frame blocks and all landmark blocks — its code is the
parent commit's. Per window: wall time per call through the Python binding (what a caller waits), on a handle without profiling,
and the device time of the kernel classes between hipEvents (cfg.profile_kernels) on a second handle.
"""
import os, sys, time
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "tests"))

STEPS = ("cov_assemble", "cov_assemble_sqrt", "cov_invert", "cov_band", "cov_band_sel", "k_cov_lmk", "cov_band_rows", "cov_cross", "cov_band_pairs", "cov_band_gather")


def timed(fn, calls):
    for _ in range(3):
        fn()
    t = time.perf_counter()
    for _ in range(calls):
        fn()
    return (time.perf_counter() - t) / calls


def measure(name, w, calls, out):
    import numpy as np
    import cov_cross_helpers as xh
    from sadvio_amd import capi
    kf = np.zeros(w.n_lmk, dtype=np.int32)
    lmk = np.arange(w.n_lmk, dtype=np.int32)
    cam = np.zeros(w.n_lmk, dtype=np.int32)
    res = {}
    for prof in (False, True):
        be = capi.Backend(device=0, profile_kernels=prof)
        be.set_windows([w])
        s = be.solve(capi.reference_options())[0]
        d = be.get_deltas(0)
        meas = np.array([xh.predicted(w, d, 0, int(l), 0) for l in lmk]) + xh.PIXEL_OFFSET
        cross = lambda: be.covariance_cross(0, kf, lmk, cam, meas, raw_rc=True)
        base = lambda: be.covariance(0, kf=list(range(w.n_kf)), lmk="all", raw_rc=True)
        r = cross()
        if not prof:
            res["rc"] = r["rc"]
            res["wall_cross"] = timed(cross, calls)
            res["wall_base"] = timed(base, calls)
            res["status"] = np.bincount(r["status"], minlength=3)
        else:
            for _ in range(3):
                cross()
            kt = be.kernel_times()
            res["cross_steps"] = ", ".join(f"{k} {kt[k]['avg_us']:.1f} us" for k in STEPS if k in kt)
            be.close()
            be = capi.Backend(device=0, profile_kernels=True)
            be.set_windows([w]); be.solve(capi.reference_options())
            for _ in range(4):
                base()
            kt = be.kernel_times()
            res["base_steps"] = ", ".join(f"{k} {kt[k]['avg_us']:.1f} us" for k in STEPS if k in kt)
        be.close()
    n_free = int((w.kf_const == 0).sum())
    line = (f"{name}: {w.n_kf} KF ({n_free} free, d = {15 if w.has_imu else 6}), {w.n_lmk} landmarks, {w.n_obs} observations, solve {s.iterations} iterations; "
            f"{w.n_lmk} candidates (newest key-frame x every landmark, with innovation; rc {res['rc']}, status OK / singular / invalid projection "
            f"{res['status'][0]} / {res['status'][1]} / {res['status'][2]}); {calls} calls: covariance_cross {res['wall_cross'] * 1e6:.1f} us wall per call, "
            f"covariance (all key-frame + all landmark blocks) {res['wall_base'] * 1e6:.1f} us; device, covariance_cross: {res['cross_steps']}; "
            f"device, covariance: {res['base_steps']}")
    print(line, flush=True)
    out.write(line + "\n"); out.flush()


if __name__ == "__main__":
    calls = int(sys.argv[1]) if len(sys.argv) > 1 else 30
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    path = sys.argv[2] if len(sys.argv) > 2 else os.path.join(root, "profiles", "r20_covariance_cross_time.txt")
    from sadvio_amd import synthetic
    from vio_helpers import make_vio_window
    with open(path, "w") as out:
        measure("shipped VIO window", make_vio_window(n_kf=12, n_lmk=2900, seed=11), calls, out)
        measure("config 2", synthetic.make_window(), calls, out)
        measure("345 KF", synthetic.make_window(n_kf=345, n_lmk=9 * 345, length=172.5, band=3, seed=3), calls, out)
