#!/usr/bin/env python
"""Do two builds of the library marginalise and sparsify to the same results?  python scripts/marg_same_results.py OLD_LIB NEW_LIB

Every run is a fresh child process with SADVIO_BA_LIB set to one of the libraries and SADVIO_DEBUG=16384 (the route lines). Cases:
  unpivoted   small_vio_case(seed=75, n_lmk=500, n_lonely=12), Cholesky form, the reference's cut: the unpivoted route
  pivoted_*   small_vio_case(seed=76, ...) without a previous prior, Cholesky form, both cuts: rank deficient, pivoted, refined
  config3     config3_marg_case(300), eigen form, then sparsify of the resident prior
Discrete results (n_full, sweeps, marg_stats, the route lines without their timings, the sparsified factors' types and indices) must
be equal. The matrices (J^T J, J^T r0, the factors' sqrt_inf) are assembled with floating-point atomics: OLD is first run three times
against itself; if it is bit-identical to itself NEW must be bit-identical to it, else NEW's largest difference to OLD must stay within
twice OLD's largest difference to itself (a maximum over three repetitions underestimates the tail). Exit status 0 = same, 1 = different,
3 = a child process failed."""
import json, os, re, subprocess, sys, tempfile
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT); sys.path.insert(0, os.path.join(ROOT, "tests"))
import numpy as np


def child(out_path):
    from sadvio_amd import capi
    from golden_util import config3_marg_case
    from test_gpu_margloop import small_vio_case
    disc, mats = {}, {}

    def record(name, be, g):
        disc[name] = {"m": g["m"], "n": g["n"], "n_full": g["n_full"], "sweeps": list(g["sweeps"]), "marg_stats": be.marg_stats(),
                      "lmk_col": [int(c) for c in g["lmk_col"]]}
        mats[name + ".JtJ"] = g["J"].T @ g["J"]
        mats[name + ".Jtr0"] = g["J"].T @ g["r0"]

    w, args = small_vio_case(seed=75, n_lmk=500, n_lonely=12)
    be = capi.Backend(device=0)
    be.set_windows([w])
    record("unpivoted", be, be.marginalize(0, eig_cut="reference", form="cholesky", **args))
    be.close()
    w, args = small_vio_case(seed=76, n_lmk=500, n_lonely=12)
    args["last"] = None
    for cut in ("reference", "noise_floor"):
        be = capi.Backend(device=0)
        be.set_windows([w])
        record("pivoted_" + cut, be, be.marginalize(0, eig_cut=cut, form="cholesky", **args))
        be.close()
    w, args = config3_marg_case(300)
    be = capi.Backend(device=0)
    be.set_windows([w])
    g = be.marginalize(0, eig_cut="reference", form="eigen", **args)
    record("config3", be, g)
    fs = be.sparsify(0, {k: v for k, v in g.items() if k not in ("J", "r0")}, vio=True)
    be.close()
    disc["config3"]["factors"] = [[f["type"], f["kf"], f["lmk0"]] for f in fs]
    mats["config3.sqrt_inf"] = np.concatenate([np.asarray(f["sqrt_inf"], dtype=np.float64).ravel() for f in fs])
    np.savez(out_path, disc=json.dumps(disc, sort_keys=True), **mats)


def run(lib, tag, out_dir):
    path = os.path.join(out_dir, f"marg_same_{tag}.npz")
    env = dict(os.environ, SADVIO_BA_LIB=os.path.abspath(lib), SADVIO_DEBUG="16384")
    p = subprocess.run([sys.executable, os.path.abspath(__file__), "--child", path], env=env, capture_output=True, text=True, timeout=240)
    if p.returncode != 0:
        print(f"{tag}: the child ended with status {p.returncode}; nothing further is started\n{p.stderr[-2000:]}")
        sys.exit(3)
    z = np.load(path)   # (an .npz is read lazily: everything is taken out below, before the directory goes)
    # route lines: everything up to a wall time is the route ("... 0.123 ms" is not)
    routes = [re.sub(r"\d+\.\d+ ms", "- ms", ln) for ln in p.stderr.splitlines() if ln.startswith("[sadvio dbg]")]
    return {"disc": json.loads(str(z["disc"])), "routes": routes, "mats": {k: z[k] for k in z.files if k != "disc"}}


def max_diff(a, b):
    return {k: float(np.abs(a["mats"][k] - b["mats"][k]).max() / max(np.abs(a["mats"][k]).max(), 1e-300)) for k in a["mats"]}


def main(old_lib, new_lib):
    with tempfile.TemporaryDirectory() as out_dir:   # the children's results: read back at once, not kept
        olds = [run(old_lib, f"old{i}", out_dir) for i in range(3)]
        new = run(new_lib, "new", out_dir)
    ok = True
    for what in ("disc", "routes"):
        same_old = all(o[what] == olds[0][what] for o in olds)
        if what == "routes" and not same_old:
            # printed values (pivots, traces, rotation counts) follow the atomics' summation order: where OLD's own runs print different
            # numbers, first the %e values are masked everywhere, then every number of the lines that still differ between OLD's runs
            print("routes: OLD's printed values differ between its own runs; masking them")
            for r in olds + [new]:
                r["routes"] = [re.sub(r"-?\d\.\d+e[+-]\d+", "#", ln) for ln in r["routes"]]
            if len({len(o["routes"]) for o in olds}) == 1:
                noisy = [i for i in range(len(olds[0]["routes"])) if len({o["routes"][i] for o in olds}) > 1]
                for r in olds + [new]:
                    for i in noisy:
                        if i < len(r["routes"]): r["routes"][i] = re.sub(r"\d+", "#", r["routes"][i])
                print(f"routes: {len(noisy)} line(s) with all numbers masked")
            same_old = all(o[what] == olds[0][what] for o in olds)
        same_new = new[what] == olds[0][what]
        print(f"{what}: OLD equal to itself over 3 runs: {same_old}; NEW equal to OLD: {same_new}")
        if not same_new:
            ok = False
            a, b = olds[0][what], new[what]
            if what == "routes":
                for x, y in zip(a, b):
                    if x != y: print("  old:", x, "\n  new:", y)
                print(f"  ({len(a)} lines old, {len(b)} lines new)")
            else:
                print("  old:", json.dumps(a, sort_keys=True), "\n  new:", json.dumps(b, sort_keys=True))
    print(f"route lines compared: {len(olds[0]['routes'])}")
    d_old = {k: max(max_diff(olds[0], olds[1])[k], max_diff(olds[0], olds[2])[k], max_diff(olds[1], olds[2])[k]) for k in olds[0]["mats"]}
    d_new = {k: max(max_diff(o, new)[k] for o in olds) for k in olds[0]["mats"]}
    for k in sorted(d_old):
        bar = 2.0 * d_old[k]
        good = d_new[k] <= bar
        ok = ok and good
        print(f"{k}: max |OLD - OLD| / max|.| = {d_old[k]:.3e}   max |NEW - OLD| / max|.| = {d_new[k]:.3e}   "
              + ("bit-identical required" if bar == 0.0 else f"bar {bar:.3e}") + ("   ok" if good else "   EXCEEDED"))
    print("SAME" if ok else "DIFFERENT")
    return 0 if ok else 1


if __name__ == "__main__":
    if sys.argv[1] == "--child":
        child(sys.argv[2])
    else:
        sys.exit(main(sys.argv[1], sys.argv[2]))
