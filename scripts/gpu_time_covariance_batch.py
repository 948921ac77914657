#!/usr/bin/env python
"""Time of sadvio_ba_covariance_batch against the loop of sadvio_ba_covariance calls it replaces.

  python scripts/gpu_time_covariance_batch.py [CALLS]                      # this build
  SADVIO_BA_LIB=/path/to/parent/libsadvio_ba.so python scripts/gpu_time_covariance_batch.py [CALLS]   # a build without the batch call: the loop only

Three submissions; per window all key-frame blocks and all landmark blocks:
  8 x config 2 (20 KF x 8 000 landmarks each) on the latency path: the loop of 8 single calls, and one batch call
  64 x config 2 on the throughput path (512 000 landmarks; 8 distinct windows, each 8 times): the batch only — the single call refuses
      such a batch — beside the wall time of the solve
  8 x the shipped VIO window (12 KF with IMU states, ~2 900 landmarks, N_p = 165)
Wall time per call over CALLS calls after 3 warm-ups on a handle without profiling, through the Python binding (which allocates the
output arrays of every call afresh, for the loop and for the batch alike) and, for the batch, of the C call alone; the device time of the steps between hipEvents
(cfg.profile_kernels) on a second handle: cov_assemble | cov_invert | k_cov_lmk of the single call, covb_assemble | k_cov_inv_lds |
k_covb_lmk of the batch.
"""
import os, sys, time
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "tests"))

STEPS = ("cov_assemble", "cov_invert", "k_cov_lmk", "covb_assemble", "k_cov_inv_lds", "k_covb_lmk")


def timed(fn, calls):
    for _ in range(3):
        fn()
    t = time.perf_counter()
    for _ in range(calls):
        fn()
    return (time.perf_counter() - t) / calls


def measure(name, ws, calls, loop=True):
    from sadvio_amd import capi
    has_batch = hasattr(capi.load_library(), "sadvio_ba_covariance_batch")
    n = len(ws)
    items = [dict(w=k, kf=list(range(ws[k].n_kf)), lmk="all") for k in range(n)]
    out = {}
    for prof in (False, True):
        be = capi.Backend(device=0, profile_kernels=prof)
        be.set_windows(ws)
        t = time.perf_counter()
        s = be.solve(capi.reference_options())
        solve_first = time.perf_counter() - t
        if not prof:
            out["solve"] = timed(lambda: be.solve(capi.reference_options()), 5)
            refused = be.covariance(0, kf=[0], raw_rc=True)["rc"] != 0
            if loop and not refused:
                out["loop"] = timed(lambda: [be.covariance(k, kf=items[k]["kf"], lmk="all") for k in range(n)], calls)
            if has_batch:
                out["batch"] = timed(lambda: be.covariance_batch(items), calls)
                out["routes"] = sorted({r["route"] for r in be.covariance_batch(items)})
                arr, outs, keep = be.cov_batch_items(items)          # the C call alone, into output arrays allocated once
                out["raw"] = timed(lambda: be.lib.sadvio_ba_covariance_batch(be.h, n, arr), calls)
        else:
            refused = be.covariance(0, kf=[0], raw_rc=True)["rc"] != 0
            if loop and not refused:
                for _ in range(3):
                    [be.covariance(k, kf=items[k]["kf"], lmk="all") for k in range(n)]
            if has_batch:
                for _ in range(3):
                    be.covariance_batch(items)
            kt = be.kernel_times()
            out["steps"] = ", ".join(f"{k} {kt[k]['avg_us']:.1f} us x {kt[k]['launches'] // 3}" for k in STEPS if k in kt)
            out["lm"] = "k_lm_pass" in kt
        be.close()
    w = ws[0]
    line = (f"{name}: {n} windows of {w.n_kf} KF ({int((w.kf_const == 0).sum())} free, d = {15 if w.has_imu else 6}), {w.n_lmk} landmarks, "
            f"{w.n_obs} observations; solve by the {'throughput' if out['lm'] else 'latency'} kernels {out['solve'] * 1e3:.3f} ms wall "
            f"({s[0].iterations} iterations, first solve {solve_first * 1e3:.1f} ms)")
    if "loop" in out:
        line += f"; loop of {n} single calls {out['loop'] * 1e3:.3f} ms wall = {out['loop'] / n * 1e6:.1f} us per window"
    elif loop:
        line += "; the single call refuses this batch"
    if "batch" in out:
        line += f"; one batch call {out['batch'] * 1e3:.3f} ms wall = {out['batch'] / n * 1e6:.1f} us per window, routes {out['routes']}"
        line += f" ({out['raw'] * 1e3:.3f} ms in the C call when the output arrays are reused)"
        if "loop" in out:
            line += f"; loop / batch = {out['loop'] / out['batch']:.2f}"
    print(line + f"; device time per launch sequence (x launches per pass): {out['steps']}", flush=True)


if __name__ == "__main__":
    calls = int(sys.argv[1]) if len(sys.argv) > 1 else 50
    from sadvio_amd import capi, synthetic
    from vio_helpers import make_vio_window
    print(f"library: {capi.LIB_PATH}", flush=True)
    c2 = [synthetic.make_window(seed=20250404 + k) for k in range(8)]
    measure("8 x config 2", c2, calls)
    measure("8 x shipped VIO window", [make_vio_window(n_kf=12, n_lmk=2900, seed=11 + k) for k in range(8)], calls)
    if hasattr(capi.load_library(), "sadvio_ba_covariance_batch"):
        measure("64 x config 2", c2 * 8, max(calls // 5, 5), loop=False)
