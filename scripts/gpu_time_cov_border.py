#!/usr/bin/env python
"""Time of the covariance's border route (cov_border_kernels.h) on the 345-key-frame window with a loop closure, against the band
route on the same window without the closure factor, and the band route's figures on this build against the parent's.

  python scripts/gpu_time_cov_border.py [CALLS] [OUT]                                                 # this build: both windows
  SADVIO_BA_LIB=/path/to/parent/libsadvio_ba.so python scripts/gpu_time_cov_border.py [CALLS] [OUT]   # the parent's build: the band case only

The window is tests/cov_band_helpers.py's (345 KF, 344 free, N_p = 2 064; profiles/r18_covariance_band_time.txt's "345 KF" case);
the closure is one relative-pose factor between free key-frames 5 and 340 (tests/cov_border_helpers.py). No environment variable is
set: the window without the factor takes the band route, the one with it the border route. Request: every key-frame block, the
pairs of neighbouring key-frames, every landmark block. Three runs of each case, each on fresh handles: wall time per call over
CALLS calls after 3 warm-ups on a handle without profiling; device time per kernel class between hipEvents on a second handle. The
lines are printed and appended to OUT (default profiles/cov_border_time.txt); the spread over the three runs closes each case.
"""
import os, sys, time
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

STEPS = ("cov_assemble", "k_cov_schur", "k_cov_factors", "cov_border_split", "cov_band", "cov_band_sel", "cov_border_solve", "cov_border_schur",
         "cov_border_apply", "k_cov_lmk", "cov_band_pairs", "cov_band_gather")


def timed(fn, calls):
    for _ in range(3):
        fn()
    t = time.perf_counter()
    for _ in range(calls):
        fn()
    return (time.perf_counter() - t) / calls


def measure(w, calls):
    from sadvio_amd import capi
    free = [k for k in range(w.n_kf) if not w.kf_const[k]]
    pairs = [(free[i], free[i + 1]) for i in range(len(free) - 1)]
    out = {}
    for prof in (False, True):
        be = capi.Backend(device=0, profile_kernels=prof)
        be.set_windows([w])
        be.solve(capi.reference_options())
        call = lambda: be.covariance(0, kf=list(range(w.n_kf)), pairs=pairs, lmk="all", raw_rc=True)
        r = call()
        out["rc_prof" if prof else "rc_wall"] = r.get("rc", 0)
        if not prof:
            out["wall"] = timed(call, calls)
        else:
            for _ in range(2):
                call()
            kt = be.kernel_times()
            out["kt"] = {k: kt[k]["avg_us"] for k in STEPS if k in kt}
        be.close()
    return out


if __name__ == "__main__":
    calls = int(sys.argv[1]) if len(sys.argv) > 1 else 20
    path = sys.argv[2] if len(sys.argv) > 2 else os.path.join(ROOT, "profiles", "cov_border_time.txt")
    from sadvio_amd import capi
    import cov_band_helpers as cb
    capi.load_library()
    parent = bool(os.environ.get("SADVIO_BA_LIB"))
    cases = [("345 KF, band route", cb.window_at_size)]
    if not parent:
        import cov_border_helpers as bh
        cases.append(("345 KF + closure factor (5, 340), border route", bh.window_at_size_closure))
    lines = [f"library: {capi.LIB_PATH} ({'parent build' if parent else 'this build'}); {calls} calls per run"]
    for name, build in cases:
        w = build()
        walls = []
        for run in range(3):
            m = measure(w, calls)
            walls.append(m["wall"] * 1e3)
            lines.append(f"{name}, run {run + 1}: {m['wall'] * 1e3:.3f} ms wall per call (status {m['rc_wall']}); device time per class on the profiling handle "
                         f"(status {m['rc_prof']}): " + ", ".join(f"{k} {v:.1f} us" for k, v in m["kt"].items()))
            print(lines[-1], flush=True)
        lines.append(f"{name}: wall per call over three runs {min(walls):.3f} .. {max(walls):.3f} ms (spread {max(walls) - min(walls):.3f} ms)")
        print(lines[-1], flush=True)
    with open(path, "a") as f:
        f.write("\n".join(lines) + "\n")
