#!/usr/bin/env python
"""Do two builds of the library return the same covariances, to the bit?  python scripts/cov_same_results.py OLD_LIB NEW_LIB

Every case runs in a fresh child process of its own, once per library (SADVIO_BA_LIB), under the case's SADVIO_COV_* setting and a
time limit; the children run one at a time and nothing further is started after one that fails. A child solves with
max_num_iterations = 0 — no step is taken, so the state is the constructed one in both builds (two handles do not otherwise solve to
the same bits) — then asks for covariances, and saves get_deltas and every output, status, n_lmk_singular, return code and error text.
The covariance kernels have no floating-point atomics: every saved array of NEW must equal OLD's byte for byte. A case whose deltas
(or whose marginalisation prior, cases 3 and 4) differ has lost the comparison's premise and counts as a failure. The windows are
those of the covariance test helpers (tests/).
Exit status 0 = same, 1 = different, 3 = a child process failed."""
import json, os, subprocess, sys, tempfile
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT); sys.path.insert(0, os.path.join(ROOT, "tests"))
import numpy as np

CHILD_TIMEOUT = 120   # seconds; a child takes a few


# ---- the cases ------------------------------------------------------------------------------------------------------------------------
def _flat(prefix, r, keys):
    return {f"{prefix}.{k}": r[k] for k in keys if k in r}


def _batch(items):
    def run(be, ws, d):
        out = {}
        for i, r in enumerate(be.covariance_batch(items, fill=7.0)):
            out.update(_flat(f"item{i}", r, ("kf", "pair", "lmk", "status", "route", "n_lmk_singular")))
        return out
    return run


def _single(be, ws, d, w=0):
    n = ws[w].n_kf
    r = be.covariance(w, kf=list(range(n)), pairs=[(0, n - 1), (n - 1, 0), (1, 0)], lmk="all", raw_rc=True)
    return _flat("single", r, ("rc", "error", "kf", "pair", "lmk", "n_lmk_singular"))


def _cross(be, ws, d, w=0):
    import cov_cross_helpers as xh
    kf, lmk = xh._all_pairs(ws[w])
    cam, meas = xh.candidate_observations(ws[w], d[w], kf, lmk)
    r = be.covariance_cross(w, kf, lmk, cam, meas, raw_rc=True)
    return _flat("cross", r, ("rc", "error", "cross", "innov", "maha2", "status"))


def _all(w, n_kf):
    return dict(w=w, kf=list(range(n_kf)), pairs=[(0, n_kf - 1), (n_kf - 1, 0)], lmk="all")


def _plain(build, run):
    return lambda be: (build(), {}), run


def _vio(form):
    """The VIO window of tests/test_gpu_cov_batch.py::test_vio_with_the_resident_prior, marginalised on the case's own handle (the
    dense prior stays resident there). Marginalisation sums with floating-point atomics: the prior it made is part of the premise."""
    def prepare(be):
        import dataclasses
        import cov_helpers as ch
        w, args, w2, keep = ch.vio_marg_step()
        be.set_prior(ch.VIO_J0, np.zeros(15))
        be.set_windows([w])
        g = be.marginalize(0, form="cholesky", readback=True, **args)
        resident = dict({k: v for k, v in g.items() if k not in ("J", "r0")}, resident=True)
        fs = be.sparsify(0, resident, vio=True) if form == "sparse" else None
        w_dev = ch.vio_attach(w, w2, keep, g, fs)
        premise = {"premise.J": g["J"], "premise.r0": g["r0"]}
        if form == "dense":
            w_dev = dataclasses.replace(w_dev, dense_prior=dict({k: v for k, v in w_dev.dense_prior.items() if k not in ("J", "r0")}, resident=True))
        else:
            premise["premise.sqrt_inf"] = np.concatenate([np.asarray(f["sqrt_inf"], dtype=np.float64).ravel() for f in fs])
        return [w_dev], premise
    return prepare


def _unanchored():
    from sadvio_amd import synthetic
    wu = synthetic.make_window(n_kf=4, n_lmk=60, obs_per_lmk=4, seed=33, fixed=0)   # (tests/test_gpu_cov_batch.py::test_per_item_status)
    wu.pose_priors = []
    return [wu]


ENV = {   # case -> the SADVIO_COV_* setting of its children
    "01_batch_pixel_vo": {}, "02_batch_angular": {}, "03_batch_vio_dense_prior": {}, "04_batch_vio_sparse_prior": {}, "05_batch_lmk16": {},
    "06_batch_lmk64": {}, "07_batch_all_constant": {}, "08_batch_two_sizes_one_group": {}, "09_batch_lds_cap": {},
    "10_batch_dense_route": {"SADVIO_COV_BATCH_LDS": "0"}, "11_single_band": {"SADVIO_COV_BAND": "1"}, "12_single_sqrt": {"SADVIO_COV_SQRT": "1"},
    "13_single_long_track": {}, "14_single_not_usable": {}, "15_cross_innovation": {},
}
FLAGS = {"13_single_long_track": dict(long_tracks=True, long_track_covariance=True)}


def cases():
    """case -> (prepare(be) -> (windows, what else the comparison presumes equal), run(be, windows, deltas) -> results)"""
    import cov_band_helpers as bh
    import cov_batch_helpers as cb
    import cov_helpers as ch
    import long_cov_helpers as lc
    from frontend_helpers import landmark_optimization_window
    return {
        "01_batch_pixel_vo": _plain(lambda: [ch.window_pixel_vo()], _batch([_all(0, 3), dict(w=0, lmk=[5, ch.SINGLE, 5])])),
        "02_batch_angular": _plain(lambda: [ch.window_angular_vo()], _batch([_all(0, 4)])),
        "03_batch_vio_dense_prior": (_vio("dense"), _batch([_all(0, 4)])),
        "04_batch_vio_sparse_prior": (_vio("sparse"), _batch([_all(0, 4)])),
        "05_batch_lmk16": _plain(lambda: [ch.window_lmk600()], _batch([_all(0, 8)])),                  # 7 free key-frames
        "06_batch_lmk64": _plain(lambda: [bh.window_vo12()], _batch([_all(0, 12)])),                   # 11 free key-frames
        "07_batch_all_constant": _plain(lambda: [landmark_optimization_window()], _batch([dict(w=0, kf=[0, 1], pairs=[(0, 1)], lmk="all")])),
        "08_batch_two_sizes_one_group": _plain(lambda: [ch.window_pixel_vo(), ch.window_lmk600(), bh.window_vo12()],
                                               _batch([_all(1, 8), _all(0, 3), _all(2, 12), dict(w=1, kf=[1])])),
        "09_batch_lds_cap": _plain(lambda: [cb.window("np174"), cb.window("np180")], _batch([_all(0, 30), _all(1, 31)])),
        "10_batch_dense_route": _plain(lambda: [ch.window_pixel_vo(), ch.window_lmk600()], _batch([_all(1, 8), _all(0, 3)])),
        "11_single_band": _plain(lambda: [bh.window_vo12()], _single),
        "12_single_sqrt": _plain(lambda: [ch.window_pixel_vo()], lambda be, ws, d: dict(_single(be, ws, d), **_cross(be, ws, d))),
        "13_single_long_track": _plain(lambda: [lc.window("L65")], _single),
        "14_single_not_usable": _plain(_unanchored, _single),
        "15_cross_innovation": _plain(lambda: [ch.window_pixel_vo()], _cross),
    }


def child(name, out_path):
    from sadvio_amd import capi
    prepare, run = cases()[name]
    be = capi.Backend(device=0, **FLAGS.get(name, {}))
    try:
        ws, out = prepare(be)
        be.set_windows(ws)
        o = capi.reference_options()
        o.max_num_iterations = 0
        be.solve(o)
        d = [be.get_deltas(k) for k in range(len(ws))]
        out.update(run(be, ws, d))
    finally:
        be.close()
    for k, dk in enumerate(d):
        out.update({f"premise.deltas{k}.{key}": v for key, v in dk.items() if v is not None})
    np.savez(out_path, **{k: np.asarray(v) for k, v in out.items()})


def run_child(lib, name, env, out_dir, tag):
    path = os.path.join(out_dir, f"{name}_{tag}.npz")
    full = {k: v for k, v in os.environ.items() if not k.startswith("SADVIO_COV_")}
    full.update(env, SADVIO_BA_LIB=os.path.abspath(lib))
    try:
        p = subprocess.run([sys.executable, os.path.abspath(__file__), "--child", name, path], env=full, capture_output=True, text=True, timeout=CHILD_TIMEOUT)
        status, err = p.returncode, p.stderr
    except subprocess.TimeoutExpired as e:
        status, err = 124, f"no result after {CHILD_TIMEOUT} s\n" + (e.stderr or b"").decode(errors="replace")
    if status != 0:
        print(f"{name} [{tag}]: the child ended with status {status}; nothing further is started\n{err[-3000:]}")
        sys.exit(3)
    with np.load(path) as z:
        return {k: z[k] for k in z.files}


def main(old_lib, new_lib):
    names = sorted(ENV)
    ok = True
    with tempfile.TemporaryDirectory() as out_dir:
        for name in names:
            env = ENV[name]
            old, new = run_child(old_lib, name, env, out_dir, "old"), run_child(new_lib, name, env, out_dir, "new")
            keys = sorted(set(old) | set(new))
            bad = [k for k in keys if k not in old or k not in new or old[k].dtype != new[k].dtype or old[k].shape != new[k].shape
                   or old[k].tobytes() != new[k].tobytes()]
            bad_premise = [k for k in bad if k.startswith("premise.")]
            n_bytes = sum(v.nbytes for v in old.values())
            facts = ", ".join(f"{k.split('.', 1)[1]} {old[k]}" for k in keys if k.endswith((".rc", ".status", ".route")) and old[k].ndim == 0)
            print(f"{name} {json.dumps(env) if env else ''}: {len(keys)} arrays, {n_bytes} bytes ({facts}): "
                  + ("byte-equal" if not bad else "DIFFERENT in " + ", ".join(bad))
                  + ("   [the state differs before any covariance is asked for: the premise of the comparison is lost]" if bad_premise else ""))
            for k in keys:
                if k.endswith(".error"):
                    print(f"    {k}: {str(old[k])!r}" + ("" if k not in bad else f" -> {str(new.get(k))!r}"))
            ok = ok and not bad
    print(f"{len(names)} cases: " + ("SAME" if ok else "DIFFERENT"))
    return 0 if ok else 1


if __name__ == "__main__":
    if sys.argv[1] == "--child":
        child(sys.argv[2], sys.argv[3])
    else:
        sys.exit(main(sys.argv[1], sys.argv[2]))
