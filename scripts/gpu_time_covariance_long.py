#!/usr/bin/env python
"""Time of one sadvio_ba_covariance call on a window with long tracks (profiles/r23_covariance_long_time.txt). One MI355X.

  python scripts/gpu_time_covariance_long.py [CALLS] [BLOCKS]

Window long80: 100 KF x 50 000 landmarks x 5 observations (the config-4 shape) in which every 50th landmark is a track of 80
observations, on a handle created with long_tracks and long_track_covariance; cut64: the same window with those tracks cut to 64
observations on a handle without the flags — what a caller had to do before (scripts/gpu_measure_long_track_priors.py builds both).
Every call asks for all key-frame blocks and all landmark blocks. Per window and per SADVIO_COV_SQRT (unset | 1; read when the handle
is created): wall time per call — what a caller waits, the host wait of the pivot test and the read-back included — over BLOCKS
blocks of CALLS calls after a warm-up of 3, the two windows alternating so that both see the same machine; then, on a profiling handle
of its own, the device time per launch of the classes between hipEvents on the handle's stream (cfg.profile_kernels)."""
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests"), os.path.join(ROOT, "scripts")]

CLASSES = ("cov_assemble", "cov_assemble_sqrt", "k_cov_long", "k_cov_schur", "k_cov_schur_sqrt", "cov_invert", "k_cov_lmk_long", "k_cov_lmk")


def handle(w, flags, profile=False):
    from sadvio_amd import capi
    be = capi.Backend(device=0, profile_kernels=profile, **flags)
    be.set_windows([w])
    s = be.solve(capi.gn_options(10))[0]
    return be, s


def main():
    calls = int(sys.argv[1]) if len(sys.argv) > 1 else 20
    blocks = int(sys.argv[2]) if len(sys.argv) > 2 else 3
    import numpy as np
    from gpu_measure_long_track_priors import build_window
    legs = {"long80": (build_window(False)[0], dict(long_tracks=True, long_track_covariance=True)), "cut64": (build_window(True)[0], {})}
    for name, (w, _) in legs.items():
        n = np.diff(w.lmk_obs_ptr)
        print(f"window {name}: {w.n_kf} KF ({int((w.kf_const == 0).sum())} free), {w.n_lmk} landmarks, {w.n_obs} observations, "
              f"{(n > 64).sum()} landmarks above 64 observations (max {n.max()})", flush=True)
    for sqrt in (None, "1"):
        if sqrt is None:
            os.environ.pop("SADVIO_COV_SQRT", None)
        else:
            os.environ["SADVIO_COV_SQRT"] = sqrt
        tag = f"SADVIO_COV_SQRT {'unset' if sqrt is None else '= ' + sqrt}"
        hs = {name: handle(w, flags) for name, (w, flags) in legs.items()}
        wall, last = {name: [] for name in legs}, {}
        for name, (be, _) in hs.items():
            for _ in range(3):
                c = be.covariance(0, kf=list(range(legs[name][0].n_kf)), lmk="all")
        for _ in range(blocks):
            for name, (be, _) in hs.items():
                kf = list(range(legs[name][0].n_kf))
                t = time.perf_counter()
                for _ in range(calls):
                    c = be.covariance(0, kf=kf, lmk="all")
                wall[name].append((time.perf_counter() - t) / calls * 1e3)
                last[name] = c
        for name, (be, s) in hs.items():
            be.close()
            print(f"{tag}: {name}: solve {s.iterations} iterations, cost {s.initial_cost:.6g} -> {s.final_cost:.6g}; {blocks} blocks of {calls} calls, wall per call "
                  + " | ".join(f"{v:.3f}" for v in wall[name]) + f" ms (median {sorted(wall[name])[len(wall[name]) // 2]:.3f} ms); singular landmarks {last[name]['n_lmk_singular']}", flush=True)
        for name, (w, flags) in legs.items():
            be, _ = handle(w, flags, profile=True)
            for _ in range(3 + calls):
                be.covariance(0, kf=list(range(w.n_kf)), lmk="all")
            kt = be.kernel_times()
            be.close()
            print(f"{tag}: {name}: device, us per launch: " + ", ".join(f"{k} {kt[k]['avg_us']:.1f} (x{kt[k]['launches']})" for k in CLASSES if k in kt), flush=True)


if __name__ == "__main__":
    main()
