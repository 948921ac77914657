#!/usr/bin/env python
"""Times of the batch calls on windows with long tracks (profiles/long_batch_time.txt). One MI355X.

  python scripts/gpu_time_long_batch.py [--calls N] [--runs R] [--cut-only] [--out FILE]

(a) sadvio_ba_covariance_batch of 8 copies of W300 (tests/long_cov_helpers.py: 300 key-frames, 10 free, one track of 600 observations
    among 60 short ones; N_p = 60, the LDS route), every item asking for all key-frame blocks and all landmark blocks, against the loop
    of 8 sadvio_ba_covariance calls on the same handle (flags SADVIO_CFG_LONG_TRACKS | _COVARIANCE | _BATCH). Wall time per call of
    either kind over R runs of N calls after a warm-up of 3, the two kinds alternating; then, on a profiling handle, the device time per
    launch of the kernel classes.
(b) sadvio_ba_marginalize_relative_batch over all pairs (k, k + 1), (k, k + 2) of long80 (scripts/gpu_measure_long_track_priors.py: 100
    key-frames x 50 000 landmarks, every 50th a track of 80 observations; flags SADVIO_CFG_LONG_TRACKS | _BATCH) and of cut64 (the same
    window with those tracks cut to 64 observations, a handle without flags: what a caller had to do before). Wall time per call over R
    runs of N calls each, the spread of the runs stated, and the device time of k_rel_batch.
--cut-only runs the cut64 leg of (b) alone: it is what a library built from the parent commit (SADVIO_BA_LIB) can run, for the
comparison of this commit against its parent on the window both serve. Every line goes to stdout and is appended to FILE."""
import argparse
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests"), os.path.join(ROOT, "scripts")]

COV_CLASSES = ("covb_assemble", "k_covb_long", "k_cov_inv_lds", "k_covb_lmk", "k_covb_lmk_long", "cov_assemble", "k_cov_long", "k_cov_schur", "cov_invert",
               "k_cov_lmk_long", "k_cov_lmk")
OUT = None


def say(line):
    print(line, flush=True)
    if OUT:
        with open(OUT, "a") as f:
            f.write(line + "\n")


def spread(v):
    return f"{' | '.join(f'{x:.3f}' for x in v)} ms (median {sorted(v)[len(v) // 2]:.3f}, spread {(max(v) - min(v)) / min(v) * 100:.1f} %)"


def classes(kt, names):
    return ", ".join(f"{k} {kt[k]['avg_us']:.1f} (x{kt[k]['launches']})" for k in names if k in kt)


def covariance_leg(calls, runs):
    import long_cov_helpers as lc
    from sadvio_amd import capi
    w = lc.w300()
    ws = [w] * 8
    flags = dict(long_tracks=True, long_track_covariance=True, long_track_batch=True)
    kf = list(range(w.n_kf))
    items = [dict(w=i, kf=kf, lmk="all") for i in range(8)]
    say(f"(a) 8 x W300: {w.n_kf} KF ({int((w.kf_const == 0).sum())} free), {w.n_lmk} landmarks, {w.n_obs} observations each, one track of 600; all key-frame and landmark blocks")
    be = capi.Backend(device=0, **flags)
    be.set_windows(ws)
    be.solve(capi.gn_options(4))
    arr, outs, keep = be.cov_batch_items(items)

    def batch():
        rc = be.lib.sadvio_ba_covariance_batch(be.h, 8, arr)
        assert rc == 0 and all(arr[i].status == 0 and arr[i].route == capi.COV_ROUTE_LDS for i in range(8)), rc

    def loop():
        for i in range(8):
            be.covariance(i, kf=kf, lmk="all")

    for _ in range(3):
        batch(); loop()
    wall = {"batch": [], "loop": []}
    for _ in range(runs):
        for name, fn in (("batch", batch), ("loop", loop)):
            t = time.perf_counter()
            for _ in range(calls):
                fn()
            wall[name].append((time.perf_counter() - t) / calls * 1e3)
    be.close()
    say(f"(a) covariance_batch, 8 items, {runs} runs of {calls} calls, wall per call: " + spread(wall["batch"]))
    say(f"(a) loop of 8 sadvio_ba_covariance, wall per loop:                    " + spread(wall["loop"]))
    for name in ("batch", "loop"):
        be = capi.Backend(device=0, profile_kernels=True, **flags)
        be.set_windows(ws)
        be.solve(capi.gn_options(4))
        for _ in range(3 + calls):
            if name == "batch":
                be.covariance_batch(items)
            else:
                for i in range(8):
                    be.covariance(i, kf=kf, lmk="all")
        kt = be.kernel_times()
        be.close()
        say(f"(a) {name}: device, us per launch: " + classes(kt, COV_CLASSES))


def relative_leg(calls, runs, cut_only):
    import numpy as np
    from gpu_measure_long_track_priors import build_window
    from sadvio_amd import capi
    legs = {"cut64": (build_window(True)[0], {})}
    if not cut_only:
        legs["long80"] = (build_window(False)[0], dict(long_tracks=True, long_track_batch=True))
    tag = os.environ.get("SADVIO_BA_LIB", "this build")
    for name, (w, flags) in legs.items():
        n = np.diff(w.lmk_obs_ptr)
        pairs = [(k, k + s) for k in range(w.n_kf - 1) for s in (1, 2) if k + s < w.n_kf]
        say(f"(b) [{tag}] window {name}: {w.n_kf} KF, {w.n_lmk} landmarks, {w.n_obs} observations, {(n > 64).sum()} landmarks above 64 observations "
            f"(max {n.max()}); {len(pairs)} pairs")
        be = capi.Backend(device=0, **flags)
        be.set_windows([w])
        for _ in range(3):
            got = be.marginalize_relative_batch(0, pairs)
        wall = []
        for _ in range(runs):
            t = time.perf_counter()
            for _ in range(calls):
                got = be.marginalize_relative_batch(0, pairs)
            wall.append((time.perf_counter() - t) / calls * 1e3)
        be.close()
        say(f"(b) [{tag}] {name}: marginalize_relative_batch, {runs} runs of {calls} calls, wall per call: " + spread(wall)
            + f"; {int((got['status'] == 0).sum())} pairs served, shared landmarks {got['n_shared'].min()} .. {got['n_shared'].max()}")
        be = capi.Backend(device=0, profile_kernels=True, **flags)
        be.set_windows([w])
        for _ in range(3 + calls):
            be.marginalize_relative_batch(0, pairs)
        kt = be.kernel_times()
        be.close()
        say(f"(b) [{tag}] {name}: device, us per launch: " + classes(kt, ("k_rel_batch",)))


def main():
    global OUT
    ap = argparse.ArgumentParser()
    ap.add_argument("--calls", type=int, default=10)
    ap.add_argument("--runs", type=int, default=3)
    ap.add_argument("--cut-only", action="store_true")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "long_batch_time.txt"))
    a = ap.parse_args()
    OUT = a.out
    if not a.cut_only:
        covariance_leg(a.calls, a.runs)
    relative_leg(a.calls, a.runs, a.cut_only)


if __name__ == "__main__":
    main()
