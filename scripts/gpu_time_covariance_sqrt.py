#!/usr/bin/env python
"""Time of the covariance's square-root assembly (cov_kernels.h: k_cov_assemble_sqrt, k_cov_schur_sqrt) against the plain one, same
build: SADVIO_COV_SQRT=0 against =1, and configs 4 / 5 with the variable unset and =1.

  python scripts/gpu_time_covariance_sqrt.py [CALLS] [vio] [config2] [kf345] [config4] [config5]        # no name: all of them

shipped VIO window (12 KF with IMU states, ~2 900 landmarks), config 2 (20 KF x 8 000 landmarks), the 345-key-frame band window of
tests/cov_band_helpers.py: sadvio_ba_covariance for all key-frame blocks, the pairs of neighbouring key-frames and every landmark
block, SADVIO_COV_SQRT=0 and =1.
Config 4 (100 KF x 50 000 landmarks; SADVIO_COV_BAND unset = dense route, and = 1) and config 5 (500 KF x 200 000 landmarks, through
sadvio_ba_covariance_batch, route BAND), after three Gauss-Newton steps and under reference options: SADVIO_COV_SQRT unset (plain
first, square-root after a refusal) and =1.
status: 0, or -2 = SADVIO_E_NOT_USABLE. Two handles do not solve to the same bits, so the status of the timed handle and of the
profiling handle are printed separately. Wall time per call over CALLS calls after 3 warm-ups on a handle without profiling, through
the Python binding; device time of the steps between hipEvents (cfg.profile_kernels) on a second handle. cov_assemble /
cov_assemble_sqrt span the whole assembly; on the band route k_cov_schur / k_cov_schur_sqrt and k_cov_factors are classes of their own
inside that span. With the variable unset a refused plain form shows both assemblies (and both inversions, averaged per class).
"""
import os, sys, time
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "tests"))

STEPS = ("cov_assemble", "k_cov_schur", "cov_assemble_sqrt", "k_cov_schur_sqrt", "k_cov_factors", "cov_invert", "cov_band", "cov_band_sel", "k_cov_lmk",
         "cov_band_pairs", "cov_band_gather")


def timed(fn, calls):
    for _ in range(3):
        fn()
    t = time.perf_counter()
    for _ in range(calls):
        fn()
    return (time.perf_counter() - t) / calls


def setenv(key, val):
    if val is None:
        os.environ.pop(key, None)
    else:
        os.environ[key] = val


def measure(name, w, calls, sqrt, band=None, batch=False, gn=0):
    from sadvio_amd import capi
    setenv("SADVIO_COV_SQRT", sqrt); setenv("SADVIO_COV_BAND", band)
    free = [k for k in range(w.n_kf) if not w.kf_const[k]]
    pairs = [(free[i], free[i + 1]) for i in range(len(free) - 1)]
    item = dict(w=0, kf=list(range(w.n_kf)), pairs=pairs, lmk="all")
    out = {}
    for prof in (False, True):
        be = capi.Backend(device=0, profile_kernels=prof)
        be.set_windows([w])
        opts = capi.gn_options(gn) if gn else capi.reference_options()
        s = be.solve(opts)
        if batch:
            call = lambda: be.covariance_batch([item])[0]
        else:
            call = lambda: be.covariance(0, kf=item["kf"], pairs=pairs, lmk="all", raw_rc=True)
        r = call()
        out["rc_prof" if prof else "rc_wall"] = r.get("status", r.get("rc", 0))
        if out["rc_prof" if prof else "rc_wall"] not in (0, capi.E_NOT_USABLE):     # a HIP error: nothing more is started on the device
            raise SystemExit(f"{name}: covariance returned {r}")
        out["route"] = r.get("route")
        if not prof:
            out["wall"] = timed(call, calls)
        else:
            for _ in range(2):
                call()
            kt = be.kernel_times()
            out["steps"] = ", ".join(f"{k} {kt[k]['avg_us']:.1f} us" for k in STEPS if k in kt)
        be.close()
    print(f"{name} [SADVIO_COV_SQRT {'unset' if sqrt is None else sqrt}, SADVIO_COV_BAND {'unset' if band is None else band}, {'batch' if batch else 'single'} call, "
          f"{'GN ' + str(gn) if gn else 'reference options'}]: {w.n_kf} KF ({len(free)} free), {w.n_lmk} landmarks, {w.n_obs} observations ({s[0].iterations} iterations)"
          + (f"; route {out['route']}" if out["route"] is not None else "") +
          f"; {len(item['kf'])} key-frame blocks, {len(pairs)} pair blocks, {w.n_lmk} landmark blocks: {out['wall'] * 1e3:.3f} ms wall per call (status {out['rc_wall']}); "
          f"device time per step on the profiling handle (status {out['rc_prof']}): {out['steps']}", flush=True)


if __name__ == "__main__":
    args = sys.argv[1:]
    calls = int(args.pop(0)) if args and args[0].isdigit() else 20
    want = set(args) or {"vio", "config2", "kf345", "config4", "config5"}
    from sadvio_amd import capi, synthetic
    print(f"library: {capi.LIB_PATH}", flush=True)
    capi.load_library()
    if "vio" in want:
        from vio_helpers import make_vio_window
        w = make_vio_window(n_kf=12, n_lmk=2900, seed=11)
        for v in ("0", "1"):
            measure("shipped VIO window", w, calls, v)
    if "config2" in want:
        w = synthetic.make_window()
        for v in ("0", "1"):
            measure("config 2", w, calls, v)
    if "kf345" in want:
        w = synthetic.make_window(n_kf=345, n_lmk=9 * 345, length=172.5, band=3, seed=3)
        for v in ("0", "1"):
            measure("345 KF", w, calls, v)
    if "config4" in want:
        w = synthetic.make_window(n_kf=100, n_lmk=50000, length=50.0, band=6, seed=4)
        for gn in (3, 0):
            for band in (None, "1"):
                for v in (None, "1"):
                    measure("config 4", w, calls, v, band=band, gn=gn)
    if "config5" in want:
        w = synthetic.make_window(n_kf=500, n_lmk=200000, length=250.0, band=6, seed=5)
        for gn in (3, 0):
            for v in (None, "1"):
                measure("config 5", w, max(calls // 4, 3), v, batch=True, gn=gn)
