#!/usr/bin/env python
"""Do two builds of the library answer the C API the same way, to the bit?  python scripts/capi_same_results.py OLD_LIB NEW_LIB

Every case runs in a fresh child process of its own, once per library (SADVIO_BA_LIB), under a time limit; the children run one at a
time and nothing further is started after one that fails. A child saves every output array, return code, summary field and last_error
text of its calls; every saved array of NEW must equal OLD's byte for byte. No case takes an LM step: a step sums with floating-point
atomics, and two handles do not solve to the same bits. The windows are the smallest the helpers under tests/ make. Cases:

  vi_init (5 frames, tests/viinit_helpers.py)
    01_viinit_bias            optim_bias with prior sigmas          02_viinit_scale          optim_scale
    03_viinit_empty           no factor                             04_viinit_not_pd         a covariance that is not positive definite
  nofov_scale (tests/nofov_helpers.py, at most 6 landmarks)
    05_nofov_usable           a usable problem                      06_nofov_lambda_out      the motion's translation at half the truth: lambda = 2 leaves [0.5, 1.5]
    07_nofov_rule             fix_scale = -1 with rotations of 0.049 / 0.051 rad and translations of 0.009 / 0.011
    08_nofov_no_landmark      n_lmk = 0 with a free scale
  linearize, landmark_chi2, landmark_chi2_models (4 key-frames, 40 landmarks), each with and without deltas
    09_gate_pixel  10_gate_angular     obs_uv given and NULL
    11_gate_twin_cameras               two cameras stored as one that disagree on image size (both chi2 calls refuse)
    12_gate_window_1                   at window index 1 of a batch of two
  a window solve with max_num_iterations = 0 after each moved setter, then get_deltas, get_trace, get_ids (4 key-frames, 40 landmarks)
    13_set_pose_priors  14_set_imu_factors  15_set_dense_prior  16_set_resident_prior  17_set_sparse_priors  18_set_lines
    19_set_in_one_update   (sparse priors and lines between begin_update and commit_update)
  20_refusals   the return code and last_error text of every entry point of include/sadvio_ba.h that takes a handle, called with a
                NULL handle, on a fresh handle, between begin_update and commit_update, on an uploaded but unsolved handle, with
                window -1 and window n_windows, and with a NULL in each pointer argument that is checked; sadvio_ba_create with each
                long-track flag alone (the text read through sadvio_ba_last_error(NULL)). The calls of the sweep are refused or trivial
                (empty lists, zero iterations): the work of each entry point is what the cases above compare.
Exit status 0 = same, 1 = different, 3 = a child process failed."""
import ctypes as C, os, subprocess, sys, tempfile
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT); sys.path.insert(0, os.path.join(ROOT, "tests"))
import numpy as np

CHILD_TIMEOUT = 120   # seconds; a child takes a few


# ---- helpers of the children ----------------------------------------------------------------------------------------------------------
def _summary(prefix, s):
    return {f"{prefix}.summary.{k}": getattr(s, k) for k, _ in s._fields_}


def _err(be):
    msg = be.lib.sadvio_ba_last_error(be.h)
    return msg.decode() if msg else ""


def _small_window(seed=11, factor=None, **kw):
    from sadvio_amd import capi, synthetic
    return synthetic.make_window(n_kf=4, n_lmk=40, obs_per_lmk=4, seed=seed, factor=capi.FACTOR_PIXEL if factor is None else factor, **kw)


def _small_vio(seed=6):
    from vio_helpers import make_vio_window
    return make_vio_window(n_kf=4, n_lmk=40, obs_per_lmk=4, seed=seed)


def _zero_iterations():
    from sadvio_amd import capi
    o = capi.reference_options()
    o.max_num_iterations = 0
    return o


# ---- vi_init ---------------------------------------------------------------------------------------------------------------------------
def _viinit(**kw):
    def inputs():
        from viinit_helpers import make_viinit
        pb = make_viinit(n_kf=5, scale=0.7, tilt=(-0.03, 0.06), vel_noise=0.01, seed=5)
        factors = [dict(f) for f in pb["factors"]]
        if kw.get("empty"): factors = []
        if kw.get("not_pd"):
            cov = np.array(factors[1]["cov"], dtype=np.float64).reshape(9, 9).copy(); cov[4, 4] = -cov[4, 4]
            factors[1]["cov"] = cov.ravel()
        return pb, factors

    def run(inp):
        from sadvio_amd import capi
        pb, factors = inp
        be = capi.Backend(device=0)
        P, keep = capi.make_viinit_problem(pb["T_f_w"], pb["vel"], factors, **{k: v for k, v in kw.items() if k not in ("empty", "not_pd")})
        s = capi.SolveSummary(); r = capi.ViInitResultC(); dv = np.full((P.n_frames, 3), 7.0)
        rc = be.lib.sadvio_ba_vi_init(be.h, C.byref(P), C.byref(capi.viinit_options()), C.byref(s), C.byref(r), capi._ptr(dv))
        out = {"rc": rc, "error": _err(be), "dv": dv, "result": np.frombuffer(bytes(r), dtype=np.uint8)}
        out.update(_summary("viinit", s))
        be.close()
        return out
    return inputs, run


# ---- nofov_scale -----------------------------------------------------------------------------------------------------------------------
def _motion(angle, t_norm):
    c, s = np.cos(angle), np.sin(angle)
    return np.concatenate([np.array([[c, -s, 0], [s, c, 0], [0, 0, 1.0]]).ravel(), t_norm * np.array([0.6, 0.0, 0.8])])


def _nofov(variants):
    def inputs():
        import nofov_helpers as nh
        pbs = []
        for v in variants:
            pb = nh.abi(nh.make_nofov(seed=2, n_points=60, n_extra=1, max_lmk=6, info_scale=v.get("info_scale", 1.0), scale0=v.get("scale0", 1.2), fix_scale=v.get("fix_scale", 0)))
            if "motion" in v: pb["T_cam0_cam0p"] = _motion(*v["motion"])
            if v.get("no_landmark"):
                pb.update(lmk_p=np.zeros((0, 3)), scale_bearing=np.zeros((0, 3)), scale_cam=np.zeros(0, dtype=np.int32), lmk_obs_ptr=np.zeros(1, dtype=np.int32),
                          obs_frame=np.zeros(0, dtype=np.int32), obs_cam=np.zeros(0, dtype=np.int32), obs_bearing=np.zeros((0, 3)))
            pbs.append(pb)
        return pbs

    def run(pbs):
        from sadvio_amd import capi
        be = capi.Backend(device=0)
        out = {}
        for i, pb in enumerate(pbs):
            r = be.nofov_scale(raw_rc=True, **pb)
            out.update({f"p{i}.{k}": r[k] for k in ("rc", "lambda", "usable", "scale_fixed", "n_inliers", "lmk_delta", "gate_norm", "inlier")})
            out.update(_summary(f"p{i}", r["summary"]))
            out[f"p{i}.error"] = _err(be)
        be.close()
        return out
    return inputs, run


# ---- linearize and the two chi2 gates ----------------------------------------------------------------------------------------------------
def _gate(factor_name, twin=False, at_window_1=False):
    def inputs():
        from sadvio_amd import capi
        factor = capi.FACTOR_PIXEL if factor_name == "pixel" else capi.FACTOR_ANGULAR
        w = _small_window(seed=12, factor=factor)
        if twin:   # camera 1 becomes a copy of camera 0: the layout stores them once
            w.cam_K[1] = w.cam_K[0]; w.cam_T_s_f[1] = w.cam_T_s_f[0]; w.cam_sigma[1] = w.cam_sigma[0]
        ws = [_other_window(factor), w] if at_window_1 else [w]
        rng = np.random.default_rng(5)
        deltas = (0.004 * rng.standard_normal((w.n_kf, 6)), 0.01 * rng.standard_normal((w.n_lmk, 3)))
        uv = rng.uniform(20.0, 400.0, (w.n_obs, 2))
        return ws, deltas, uv

    def run(inp):
        from sadvio_amd import capi
        import camera_models as cm
        ws, deltas, uv = inp
        wi = len(ws) - 1
        w = ws[wi]
        be = capi.Backend(device=0)
        be.set_windows(ws)
        out = {}
        wh = np.array([[752.0, 480.0]] * w.n_cam)
        if twin: wh[1] = (640.0, 480.0)
        models = [{"kind": cm.PINHOLE, "width": wh[c][0], "height": wh[c][1]} for c in range(w.n_cam)]
        fish = [dict(m, kind=cm.EQUIDISTANT if c == 0 else cm.PINHOLE) for c, m in enumerate(models)]
        for tag, (pd, ld) in (("zero", (None, None)), ("delta", deltas)):
            r, Jp, Jl = be.linearize(wi, pd, ld)
            out.update({f"{tag}.lin.r": r, f"{tag}.lin.Jp": Jp, f"{tag}.lin.Jl": Jl})
            for name, call in (("chi2", lambda: be.landmark_chi2(wi, pd, ld)), ("chi2_wh", lambda: be.landmark_chi2(wi, pd, ld, image_wh=wh, pixel_sigma=1.5))):
                try:
                    avg, inl = call()
                    out.update({f"{tag}.{name}.avg": avg, f"{tag}.{name}.inlier": inl})
                except capi.SadvioError as e:
                    out[f"{tag}.{name}.error"] = str(e)
            for name, (mods, u) in (("models", (models, None)), ("models_uv", (models, uv)), ("fisheye_uv", (fish, uv))):
                rc, avg, inl, obs = be.landmark_chi2_models(wi, mods, pd, ld, obs_uv=u, pixel_sigma=0.0 if u is None else 2.0, want_obs=True, raw_rc=True)
                out.update({f"{tag}.{name}.rc": rc, f"{tag}.{name}.avg": avg, f"{tag}.{name}.inlier": inl, f"{tag}.{name}.obs": obs, f"{tag}.{name}.error": _err(be)})
        be.close()
        return out
    return inputs, run


def _other_window(factor):
    from sadvio_amd import synthetic
    return synthetic.make_window(n_kf=5, n_lmk=30, obs_per_lmk=3, seed=14, factor=factor)   # the window in front: other counts at every index


# ---- a zero-iteration solve after each setter ---------------------------------------------------------------------------------------------
def _setter(what):
    def inputs():
        from line_helpers import add_lines
        from sparse_helpers import vio_sparse_priors
        from test_gpu_prior import random_prior
        w = _small_vio()
        before = None
        if what == "pose_priors": w = _small_window(seed=15, fixed=0)   # (make_window anchors an unanchored window with pose priors)
        if what in ("dense_prior", "resident_prior"): w.dense_prior = random_prior(w, 6, w.n_kf - 2, np.random.default_rng(2))
        if what == "resident_prior":
            before = (w.dense_prior["J"], w.dense_prior["r0"])
            w.dense_prior = dict({k: v for k, v in w.dense_prior.items() if k not in ("J", "r0")}, resident=True)
        if what in ("sparse_priors", "in_one_update"): w.sparse_priors = vio_sparse_priors(w, w.n_kf - 2, list(range(0, 40, 7)), np.random.default_rng(3))
        if what == "lines": w = add_lines(w, n_line=4, n_const=1)
        if what == "in_one_update": w = add_lines(w, n_line=3, n_const=1)
        return w, before

    def run(inp):
        from sadvio_amd import capi
        w, before = inp
        be = capi.Backend(device=0)
        if before is not None: be.set_prior(*before)
        be.set_windows([w], one_build=what == "in_one_update")
        sums = (capi.SolveSummary * 1)()
        out = {"solve.rc": be.lib.sadvio_ba_solve(be.h, C.byref(_zero_iterations()), sums), "solve.error": _err(be)}
        out.update(_summary("solve", sums[0]))
        out.update({f"deltas.{k}": v for k, v in be.get_deltas(0).items()})
        out["trace"] = be.get_trace(0)
        out["kf_id"], out["lmk_id"] = be.get_ids(0)
        if w.lines is not None: out["line_deltas"] = be.get_line_deltas(0, len(w.lines["T_w_l"]))
        be.close()
        return out
    return inputs, run


# ---- the refusal sweep ----------------------------------------------------------------------------------------------------------------------
def _refusals():
    def inputs():
        return _small_window(seed=16)

    def run(w):
        from sadvio_amd import capi
        import camera_models as cm
        lib = capi.load_library()
        dp, ip, lp = C.POINTER(C.c_double), C.POINTER(C.c_int32), C.POINTER(C.c_int64)
        D = np.zeros(1 << 16); I = np.zeros(1 << 16, dtype=np.int32); L = np.zeros(1 << 12, dtype=np.int64)
        d, i_, l_ = D.ctypes.data_as(dp), I.ctypes.data_as(ip), L.ctypes.data_as(lp)
        nd, ni = dp(), ip()
        arr = (capi.FlatWindowC * 1)(); arr[0] = w.to_c()
        opts0 = _zero_iterations()
        sums = (capi.SolveSummary * 4)()
        one = C.c_int32(0)
        info = capi.PriorInfoC()
        models = capi.camera_models_c([{"kind": cm.PINHOLE, "width": 752.0, "height": 480.0}] * w.n_cam)
        pr = (capi.PosePriorC * 1)(); imu = (capi.ImuFactorC * 1)(); sp = (capi.SparsePriorC * 4)()
        rq = capi.MargRequestC(); res = capi.MargResultC()
        crq = capi.CovRequestC(); xrq = capi.CovCrossRequestC()
        items = (capi.CovBatchItemC * 1)()
        vp = capi.ViInitProblemC(); np_ = capi.NoFovProblemC()
        id128 = C.create_string_buffer(128)
        NOFN = capi.ALLREDUCE_FN()
        vs, vr, ns, nr = capi.SolveSummary(), capi.ViInitResultC(), capi.SolveSummary(), capi.NoFovResultC()

        def item_w(wi):
            items[0].w = wi
            return items

        # entry point -> call(h, w): arguments that are refused, or trivial (empty lists; zero iterations)
        E = {
            "set_lines": lambda h, wi: lib.sadvio_ba_set_lines(h, wi, None),
            "get_line_deltas": lambda h, wi: lib.sadvio_ba_get_line_deltas(h, wi, d),
            "set_pose_priors": lambda h, wi: lib.sadvio_ba_set_pose_priors(h, wi, 0, None),
            "set_imu_factors": lambda h, wi: lib.sadvio_ba_set_imu_factors(h, wi, 0, None),
            "set_dense_prior": lambda h, wi: lib.sadvio_ba_set_dense_prior(h, wi, 0, 0, nd, nd, -1, 0, 0, ni, ni),
            "set_sparse_priors": lambda h, wi: lib.sadvio_ba_set_sparse_priors(h, wi, 0, None),
            "marginalize": lambda h, wi: lib.sadvio_ba_marginalize(h, wi, None, C.byref(res), i_, d, d),
            "marg_stats": lambda h, wi: lib.sadvio_ba_marg_stats(h, C.byref(one), C.byref(one), C.byref(one)),
            "get_prior": lambda h, wi: lib.sadvio_ba_get_prior(h, C.byref(info), nd, nd),
            "set_prior": lambda h, wi: lib.sadvio_ba_set_prior(h, 0, 0, 0, nd, nd),
            "marginalize_relative": lambda h, wi: lib.sadvio_ba_marginalize_relative(h, wi, 0, 0, 0, d, d),
            "marginalize_relative_batch": lambda h, wi: lib.sadvio_ba_marginalize_relative_batch(h, wi, -1, i_, i_, 0, d, d, d, i_, i_),
            "sparsify": lambda h, wi: lib.sadvio_ba_sparsify(h, wi, 0, 0, 0, nd, -1, 0, 0, ni, ni, C.byref(one), None),
            "set_collective": lambda h, wi: lib.sadvio_ba_set_collective(h, 0, 1, NOFN, None),
            "comm_init_rccl": lambda h, wi: lib.sadvio_ba_comm_init_rccl(h, 0, 0, id128),
            "comm_info": lambda h, wi: lib.sadvio_ba_comm_info(h, C.byref(one), C.byref(one), C.byref(one), C.byref(one)),
            "get_deltas": lambda h, wi: lib.sadvio_ba_get_deltas(h, wi, d, nd, nd, nd, nd),
            "get_trace": lambda h, wi: lib.sadvio_ba_get_trace(h, wi, 0, nd, C.byref(one)),
            "get_ids": lambda h, wi: lib.sadvio_ba_get_ids(h, wi, lp(), lp()),
            "linearize": lambda h, wi: lib.sadvio_ba_linearize(h, wi, nd, nd, d, nd, nd),
            "landmark_chi2": lambda h, wi: lib.sadvio_ba_landmark_chi2(h, wi, nd, nd, nd, 0.0, d, i_),
            "landmark_chi2_models": lambda h, wi: lib.sadvio_ba_landmark_chi2_models(h, wi, nd, nd, models, nd, 0.0, d, i_, nd),
            "vi_init": lambda h, wi: lib.sadvio_ba_vi_init(h, None, C.byref(opts0), C.byref(vs), C.byref(vr), nd),
            "nofov_scale": lambda h, wi: lib.sadvio_ba_nofov_scale(h, None, C.byref(opts0), C.byref(ns), C.byref(nr), nd, nd, ni),
            "covariance": lambda h, wi: lib.sadvio_ba_covariance(h, wi, C.byref(crq), nd, nd, nd, ni),
            "covariance_batch": lambda h, wi: lib.sadvio_ba_covariance_batch(h, 1, item_w(wi)),
            "covariance_cross": lambda h, wi: lib.sadvio_ba_covariance_cross(h, wi, C.byref(xrq), nd, nd, nd, ni),
            "get_kernel_times": lambda h, wi: lib.sadvio_ba_get_kernel_times(h, 0, None, nd, lp()),
            "solve": lambda h, wi: lib.sadvio_ba_solve(h, C.byref(opts0), sums),
        }
        TAKES_W = [k for k in E if k not in ("marg_stats", "get_prior", "set_prior", "set_collective", "comm_init_rccl", "comm_info", "vi_init", "nofov_scale",
                                             "get_kernel_times", "solve")]
        out = {}

        def text(h):
            msg = lib.sadvio_ba_last_error(h)
            return msg.decode() if msg else ""

        def record(tag, h, rc):
            out[f"{tag}.rc"] = rc
            out[f"{tag}.error"] = text(h)

        def create(flags=0):
            cfg = capi.Config(device=0, profile_kernels=0, use_graph=0, reserved=flags)
            h = C.c_void_p()
            return lib.sadvio_ba_create(C.byref(cfg), C.byref(h)), h

        def sweep(tag, h, names, wi=0):
            for k in names: record(f"{tag}.{k}", h, E[k](h, wi))

        # create with each long-track flag alone
        for flag in (capi.CFG_LONG_TRACK_PRIORS, capi.CFG_LONG_TRACK_COVARIANCE, capi.CFG_LONG_TRACK_BATCH):
            rc, h = create(flag)
            record(f"create.flag{flag}", None, rc)
            out[f"create.flag{flag}.handle_is_null"] = not h.value
        # a NULL handle
        for k in E: out[f"null_handle.{k}.rc"] = E[k](None, 0)
        out["null_handle.set_windows.rc"] = lib.sadvio_ba_set_windows(None, 1, arr)
        out["null_handle.begin_update.rc"] = lib.sadvio_ba_begin_update(None)
        out["null_handle.commit_update.rc"] = lib.sadvio_ba_commit_update(None)
        rc, h = create()   # (a successful create leaves no text behind)
        record("null_handle.last_error", None, rc)
        lib.sadvio_ba_destroy(None)
        # a fresh handle
        sweep("fresh", h, [k for k in E if k != "set_collective"])
        record("fresh.commit_update", h, lib.sadvio_ba_commit_update(h))
        record("fresh.set_windows_null", h, lib.sadvio_ba_set_windows(h, 1, None))
        record("fresh.set_windows_none", h, lib.sadvio_ba_set_windows(h, 0, arr))
        record("fresh.set_collective", h, E["set_collective"](h, 0))
        record("fresh.set_collective_no_callback", h, lib.sadvio_ba_set_collective(h, 0, 2, NOFN, None))
        lib.sadvio_ba_destroy(h)
        # between begin_update and commit_update
        rc, h = create()
        record("deferred.begin_update", h, lib.sadvio_ba_begin_update(h))
        record("deferred.set_windows", h, lib.sadvio_ba_set_windows(h, 1, arr))
        sweep("deferred", h, list(E))
        record("deferred.commit_update", h, lib.sadvio_ba_commit_update(h))
        lib.sadvio_ba_destroy(h)
        # uploaded, not solved (solve comes last: it changes the state)
        rc, h = create()
        record("unsolved.set_windows", h, lib.sadvio_ba_set_windows(h, 1, arr))
        sweep("unsolved", h, [k for k in E if k != "solve"])
        sweep("unsolved", h, ["solve"])
        # ... now solved: window -1 and window n_windows, then a NULL in each checked pointer argument
        for wi in (-1, 1): sweep(f"window{wi}", h, TAKES_W, wi)
        N = {
            "set_windows": lambda: lib.sadvio_ba_set_windows(h, 1, None),
            "get_line_deltas": lambda: lib.sadvio_ba_get_line_deltas(h, 0, nd),
            "set_pose_priors": lambda: lib.sadvio_ba_set_pose_priors(h, 0, 1, None),
            "set_imu_factors": lambda: lib.sadvio_ba_set_imu_factors(h, 0, 1, None),
            "set_sparse_priors": lambda: lib.sadvio_ba_set_sparse_priors(h, 0, 1, None),
            "set_dense_prior.J": lambda: lib.sadvio_ba_set_dense_prior(h, 0, 2, 15, nd, d, 0, 0, 0, ni, ni),
            "set_dense_prior.r0": lambda: lib.sadvio_ba_set_dense_prior(h, 0, 2, 15, d, nd, 0, 0, 0, ni, ni),
            "set_dense_prior.lmk_index": lambda: lib.sadvio_ba_set_dense_prior(h, 0, 2, 18, d, d, 0, 0, 1, ni, i_),
            "set_dense_prior.resident_J": lambda: lib.sadvio_ba_set_dense_prior(h, 0, capi.PRIOR_RESIDENT, 0, d, nd, 0, 0, 0, ni, ni),
            "marginalize.rq": lambda: lib.sadvio_ba_marginalize(h, 0, None, C.byref(res), i_, d, d),
            "marginalize_relative.inf36": lambda: lib.sadvio_ba_marginalize_relative(h, 0, 0, 1, 0, nd, d),
            "marginalize_relative_batch.kf_a": lambda: lib.sadvio_ba_marginalize_relative_batch(h, 0, 1, ni, i_, 0, d, d, d, i_, i_),
            "marginalize_relative_batch.inf36": lambda: lib.sadvio_ba_marginalize_relative_batch(h, 0, 1, i_, i_, 0, nd, d, d, i_, i_),
            "marginalize_relative_batch.status": lambda: lib.sadvio_ba_marginalize_relative_batch(h, 0, 1, i_, i_, 0, d, d, d, i_, ni),
            "sparsify.n_out": lambda: lib.sadvio_ba_sparsify(h, 0, 0, 0, 0, nd, -1, 0, 0, ni, ni, None, sp),
            "sparsify.out": lambda: lib.sadvio_ba_sparsify(h, 0, 0, 0, 0, nd, -1, 0, 0, ni, ni, C.byref(one), None),
            "sparsify.lmk_index": lambda: lib.sadvio_ba_sparsify(h, 0, 0, 0, 0, nd, -1, 0, 1, ni, i_, C.byref(one), sp),
            "set_prior.J": lambda: lib.sadvio_ba_set_prior(h, 2, 2, 0, nd, d),
            "get_prior.no_prior": lambda: lib.sadvio_ba_get_prior(h, C.byref(info), d, nd),
            "get_trace.rows8": lambda: lib.sadvio_ba_get_trace(h, 0, 1, nd, C.byref(one)),
            "landmark_chi2_models.models": lambda: lib.sadvio_ba_landmark_chi2_models(h, 0, nd, nd, None, nd, 0.0, d, i_, nd),
            "vi_init.opts": lambda: lib.sadvio_ba_vi_init(h, C.byref(vp), None, C.byref(vs), C.byref(vr), nd),
            "nofov_scale.opts": lambda: lib.sadvio_ba_nofov_scale(h, C.byref(np_), None, C.byref(ns), C.byref(nr), nd, nd, ni),
            "nofov_scale.arrays": lambda: lib.sadvio_ba_nofov_scale(h, C.byref(np_), C.byref(opts0), C.byref(ns), C.byref(nr), nd, nd, ni),
            "covariance.rq": lambda: lib.sadvio_ba_covariance(h, 0, None, nd, nd, nd, ni),
            "covariance_batch.items": lambda: lib.sadvio_ba_covariance_batch(h, 1, None),
            "covariance_cross.rq": lambda: lib.sadvio_ba_covariance_cross(h, 0, None, nd, nd, nd, ni),
            "comm_init_rccl.id": lambda: lib.sadvio_ba_comm_init_rccl(h, 0, 1, None),
            "comm_init_rccl.uploaded": lambda: lib.sadvio_ba_comm_init_rccl(h, 0, 1, id128),
            "set_collective.uploaded": lambda: lib.sadvio_ba_set_collective(h, 0, 1, NOFN, None),
        }
        for k, call in N.items(): record(f"null.{k}", h, call())
        lib.sadvio_ba_destroy(h)
        return out
    return inputs, run


CASES = {
    "01_viinit_bias": _viinit(optim_bias=True, sigma_dba=0.05, sigma_dbg=0.01),
    "02_viinit_scale": _viinit(optim_scale=True),
    "03_viinit_empty": _viinit(optim_scale=True, empty=True),
    "04_viinit_not_pd": _viinit(optim_scale=True, not_pd=True),
    "05_nofov_usable": _nofov([{}]),
    "06_nofov_lambda_out": _nofov([{"scale0": 0.5, "info_scale": 0.0}]),
    "07_nofov_rule": _nofov([{"fix_scale": -1, "motion": m} for m in ((0.049, 1.0), (0.051, 1.0), (0.2, 0.009), (0.2, 0.011))]),
    "08_nofov_no_landmark": _nofov([{"no_landmark": True}]),
    "09_gate_pixel": _gate("pixel"),
    "10_gate_angular": _gate("angular"),
    "11_gate_twin_cameras": _gate("pixel", twin=True),
    "12_gate_window_1": _gate("pixel", at_window_1=True),
    "13_set_pose_priors": _setter("pose_priors"),
    "14_set_imu_factors": _setter("imu_factors"),
    "15_set_dense_prior": _setter("dense_prior"),
    "16_set_resident_prior": _setter("resident_prior"),
    "17_set_sparse_priors": _setter("sparse_priors"),
    "18_set_lines": _setter("lines"),
    "19_set_in_one_update": _setter("in_one_update"),
    "20_refusals": _refusals(),
}


def child(name, out_path):
    inputs, run = CASES[name]
    inp = inputs()
    if out_path == "--inputs-only":   # builds the case's inputs without a device
        return
    np.savez(out_path, **{k: np.asarray(v) for k, v in run(inp).items()})


def run_child(lib, name, out_dir, tag):
    path = os.path.join(out_dir, f"{name}_{tag}.npz")
    full = dict(os.environ, SADVIO_BA_LIB=os.path.abspath(lib))
    try:
        p = subprocess.run(["timeout", "-k", "10", str(CHILD_TIMEOUT), sys.executable, os.path.abspath(__file__), "--child", name, path], env=full, capture_output=True, text=True)
        status, err = p.returncode, p.stderr
    except OSError as e:
        status, err = 127, str(e)
    if status != 0:
        print(f"{name} [{tag}]: the child ended with status {status}; nothing further is started\n{err[-3000:]}")
        sys.exit(3)
    with np.load(path) as z:
        return {k: z[k] for k in z.files}


def main(old_lib, new_lib, only=None):
    names = [n for n in sorted(CASES) if not only or n in only]
    ok = True
    with tempfile.TemporaryDirectory() as out_dir:
        for name in names:
            old, new = run_child(old_lib, name, out_dir, "old"), run_child(new_lib, name, out_dir, "new")
            keys = sorted(set(old) | set(new))
            bad = [k for k in keys if k not in old or k not in new or old[k].dtype != new[k].dtype or old[k].shape != new[k].shape
                   or old[k].tobytes() != new[k].tobytes()]
            codes = sorted({int(old[k]) for k in keys if k.endswith(".rc") or k == "rc"})
            texts = sorted({str(old[k]) for k in keys if k.endswith("error") and str(old[k])})
            print(f"{name}: {len(keys)} arrays, {sum(v.nbytes for v in old.values())} bytes, return codes {codes}, {len(texts)} distinct texts: "
                  + ("byte-equal" if not bad else "DIFFERENT in " + ", ".join(bad)))
            for k in bad:
                if k in old and k in new and (k.endswith("error") or k.endswith("rc")): print(f"    {k}: {str(old[k])!r} -> {str(new[k])!r}")
            if os.environ.get("CAPI_SAME_VERBOSE"):
                for t in texts: print(f"    {t!r}")
            ok = ok and not bad
    print(f"{len(names)} cases: " + ("SAME" if ok else "DIFFERENT"))
    return 0 if ok else 1


if __name__ == "__main__":
    if sys.argv[1] == "--child":
        child(sys.argv[2], sys.argv[3])
    else:
        sys.exit(main(sys.argv[1], sys.argv[2], sys.argv[3:]))
