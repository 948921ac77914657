#!/usr/bin/env python
"""Time of the covariance's band route (cov_band_kernels.h) against the dense route, and at BASELINE config 5.

  python scripts/gpu_time_covariance_band.py [CALLS]                                               # this build
  SADVIO_BA_LIB=/path/to/parent/libsadvio_ba.so python scripts/gpu_time_covariance_band.py [CALLS]  # the parent's build: config 4, dense route only

Config 4 (100 KF x 50 000 landmarks, N_p = 594, served by both routes): sadvio_ba_covariance for all key-frame blocks, the pairs of
neighbouring key-frames and every landmark block, with SADVIO_COV_BAND unset (dense route) and = 1 (band route).
Config 5 (500 KF x 200 000 landmarks, N_p = 2 994, solved by the throughput kernels): sadvio_ba_covariance_batch, one item, the same
request, no variable set; and once more with one pair block outside the band. Both also at the state after three Gauss-Newton steps,
and the 345-key-frame window of tests/cov_band_helpers.py (N_p = 2 064) through both calls.
status: 0, or -2 = SADVIO_E_NOT_USABLE (a pivot of S failed its test; the call then ends after the forward sweep / the factorisation).
Two handles do not solve to the same bits, so the status of the timed handle and of the profiling handle are printed separately.
Wall time per call over CALLS calls after 3 warm-ups on a handle without profiling, through the Python binding; device time of the
steps between hipEvents (cfg.profile_kernels) on a second handle. On the band route k_cov_schur and k_cov_factors are classes of
their own inside cov_assemble's span, cov_band is the forward sweep and cov_band_sel the backward one.
"""
import os, sys, time
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "tests"))

STEPS = ("cov_assemble", "k_cov_schur", "k_cov_factors", "cov_invert", "cov_band", "cov_band_sel", "k_cov_lmk", "cov_band_pairs", "cov_band_gather")


def timed(fn, calls):
    for _ in range(3):
        fn()
    t = time.perf_counter()
    for _ in range(calls):
        fn()
    return (time.perf_counter() - t) / calls


def measure(name, w, calls, band, batch, far_pair=False, gn=0):
    from sadvio_amd import capi
    if band is None:
        os.environ.pop("SADVIO_COV_BAND", None)
    else:
        os.environ["SADVIO_COV_BAND"] = band
    free = [k for k in range(w.n_kf) if not w.kf_const[k]]
    pairs = [(free[i], free[i + 1]) for i in range(len(free) - 1)] + ([(free[2], free[-3])] if far_pair else [])
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
        out["route"] = r.get("route")
        if not prof:
            out["solve"] = timed(lambda: be.solve(opts), 3)
            out["rc_wall"] = call().get("status", r.get("rc", 0))      # (the state the timed calls read: the last timed solve's)
            out["wall"] = timed(call, calls)
        else:
            for _ in range(2):
                call()
            kt = be.kernel_times()
            out["kt"] = kt
            out["steps"] = ", ".join(f"{k} {kt[k]['avg_us']:.1f} us" for k in STEPS if k in kt)
            out["lm"] = "k_lm_pass" in kt
        be.close()
    n_free = len(free)
    line = (f"{name} [SADVIO_COV_BAND {'unset' if band is None else band}, {'batch' if batch else 'single'} call, {'GN ' + str(gn) if gn else 'reference options'}]: {w.n_kf} KF ({n_free} free), "
            f"{w.n_lmk} landmarks, {w.n_obs} observations; solve by the {'throughput' if out['lm'] else 'latency'} kernels {out['solve'] * 1e3:.3f} ms wall "
            f"({s[0].iterations} iterations)" + (f"; route {out['route']}" if out["route"] is not None else "") +
            f"; {len(item['kf'])} key-frame blocks, {len(pairs)} pair blocks, {w.n_lmk} landmark blocks: {out['wall'] * 1e3:.3f} ms wall per call (status {out['rc_wall']}); "
            f"device time per step on the profiling handle (status {out['rc_prof']}): {out['steps']}")
    kt = out["kt"]
    if "cov_band" in kt:
        K = n_free * (1 if w.has_imu == 0 else 3)
        line += (f"; per block column ({K} of them): forward {kt['cov_band']['avg_us'] / K:.2f} us, backward {kt['cov_band_sel']['avg_us'] / K:.2f} us")
    print(line, flush=True)


if __name__ == "__main__":
    calls = int(sys.argv[1]) if len(sys.argv) > 1 else 20
    from sadvio_amd import capi, synthetic
    print(f"library: {capi.LIB_PATH}", flush=True)
    lib = capi.load_library()
    has_band = hasattr(capi, "COV_ROUTE_BAND") and not os.environ.get("SADVIO_BA_LIB")
    c4 = synthetic.make_window(n_kf=100, n_lmk=50000, length=50.0, band=6, seed=4)
    # reference options run these badly initialised windows to the iteration limit, where single landmarks have drifted next to a
    # camera centre and the assembly's S (H_pp - sum W^T H_ll W) is no longer positive definite in float64 on either route
    # (status -2); after three Gauss-Newton steps it is, and the time of a call does not depend on the state otherwise
    for gn in (0, 3):
        measure("config 4", c4, calls, None, False, gn=gn)
        if has_band:
            measure("config 4", c4, calls, "1", False, gn=gn)
    if has_band:
        measure("config 4", c4, calls, "1", False, far_pair=True, gn=3)
        c5 = synthetic.make_window(n_kf=500, n_lmk=200000, length=250.0, band=6, seed=5)
        measure("config 5", c5, max(calls // 4, 3), None, True)
        measure("config 5", c5, max(calls // 4, 3), None, True, gn=3)
        measure("config 5", c5, max(calls // 4, 3), None, True, far_pair=True, gn=3)
        # a long window the assembly serves: tests/cov_band_helpers.py's 345 key-frames (N_p = 2 064, no variable set)
        long_w = synthetic.make_window(n_kf=345, n_lmk=9 * 345, length=172.5, band=3, seed=3)
        measure("345 KF", long_w, calls, None, False)
        measure("345 KF", long_w, calls, None, False, far_pair=True)
        measure("345 KF", long_w, calls, None, True, far_pair=True)
