#!/usr/bin/env python
"""Time of one sadvio_ba_covariance call.

  python scripts/gpu_time_covariance.py [CALLS]

Two windows: the shipped VIO window (12 KF with IMU states, ~2 900 landmarks: all key-frame blocks, all landmark blocks) and
config 2 (20 KF x 8 000 landmarks). Per window: wall time per call (what a caller waits: it includes the host wait of the pivot
test and the read-back) and the device time of the three steps between hipEvents on the handle's stream (cfg.profile_kernels:
cov_assemble | cov_invert | k_cov_lmk). Run it under rocprofv3 --kernel-trace --stats for the per-kernel split.
"""
import os, sys, time
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "tests"))


def measure(name, w, calls):
    from sadvio_amd import capi
    be = capi.Backend(device=0, profile_kernels=True)
    be.set_windows([w])
    s = be.solve(capi.reference_options())[0]
    kf = list(range(w.n_kf))
    for _ in range(3):
        c = be.covariance(0, kf=kf, lmk="all")
    t = time.perf_counter()
    for _ in range(calls):
        c = be.covariance(0, kf=kf, lmk="all")
    wall = (time.perf_counter() - t) / calls
    kt = be.kernel_times()
    be.close()
    d = c["kf"].shape[1]
    n_free = int((w.kf_const == 0).sum())
    steps = ", ".join(f"{k} {kt[k]['avg_us']:.1f} us" for k in ("cov_assemble", "cov_invert", "k_cov_lmk") if k in kt)
    print(f"{name}: {w.n_kf} KF ({n_free} free, d = {d}), {w.n_lmk} landmarks, {w.n_obs} observations, solve {s.iterations} iterations; "
          f"{calls} calls, wall {wall * 1e6:.1f} us per call; device: {steps}; singular landmarks {c['n_lmk_singular']}", flush=True)


if __name__ == "__main__":
    calls = int(sys.argv[1]) if len(sys.argv) > 1 else 50
    from sadvio_amd import synthetic
    from vio_helpers import make_vio_window
    measure("shipped VIO window", make_vio_window(n_kf=12, n_lmk=2900, seed=11), calls)
    measure("config 2", synthetic.make_window(), calls)
