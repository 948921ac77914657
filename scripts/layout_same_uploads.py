#!/usr/bin/env python
"""Do two builds of the library lay the same windows out the same way?  python scripts/layout_same_uploads.py OLD_LIB NEW_LIB

Each library runs a fixed list of layouts in ONE fresh child process, with SADVIO_BA_LIB set to it and SADVIO_DEBUG=8192: UploadBatch::flush
then prints the byte count and an FNV-1a hash of every queued item's payload (neither its destination nor the alignment gaps), and the
layout driver prints the plan's scalars. Only allocation, upload and prepare work runs; nothing is solved. Per layout the lines of the
two builds are compared as multisets (the order of the add calls is free); the lap timings are left out. The layout is integer
arithmetic and copied doubles: every line must be equal. Both libraries must carry the two debug lines (an older build: apply them as
a patch). Layouts:
  config2            the config-2 window (20 key-frames x 8 000 landmarks), every setter on its own
  vio_*              the 12-key-frame VIO window with its IMU factors, and with a dense prior / the handle's resident prior / sparse
                     priors / lines
  batch64[_lm]       64 windows, and the same with SADVIO_LM=1 (chunk tables of the throughput kernels)
  contig             the config-2 window with SADVIO_CONTIG_TILES
  update             begin_update .. commit_update around the VIO window with sparse priors and lines: one build at commit
  shard1of4          rank 1 of the config-4 window sharded four ways (a collective hook set, never called)
Exit status 0 = same, 1 = different, 3 = a child process failed."""
import collections, copy, os, subprocess, sys
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT); sys.path.insert(0, os.path.join(ROOT, "tests"))


def child():
    import numpy as np
    from sadvio_amd import capi, sharding, synthetic
    from line_helpers import add_lines
    from sparse_helpers import vio_sparse_priors
    from test_gpu_prior import random_prior
    from vio_helpers import make_vio_window

    def layout(name, windows, env=None, one_build=False, before=None):
        for k, v in (env or {}).items(): os.environ[k] = v     # the switches are read when a handle is created
        print(f"== layout {name}", file=sys.stderr, flush=True)
        be = capi.Backend(device=0)
        if before: before(be)
        be.set_windows(windows, one_build=one_build)
        be.close()
        for k in (env or {}): del os.environ[k]

    c2 = synthetic.make_window(seed=20250404)
    vio = make_vio_window(n_kf=12, n_lmk=7200, seed=6)
    layout("config2", [c2])
    layout("vio_imu", [vio])
    w = copy.deepcopy(vio); w.dense_prior = random_prior(w, 40, w.n_kf - 2, np.random.default_rng(2))
    layout("vio_dense", [w])
    J, r0 = w.dense_prior["J"], w.dense_prior["r0"]
    w = copy.deepcopy(w); w.dense_prior = {k: v for k, v in w.dense_prior.items() if k not in ("J", "r0")}
    layout("vio_resident", [w], before=lambda be: be.set_prior(J, r0))
    ws = copy.deepcopy(vio); ws.sparse_priors = vio_sparse_priors(ws, ws.n_kf - 2, list(range(0, 600, 7)), np.random.default_rng(3))
    layout("vio_sparse", [ws])
    layout("vio_lines", [add_lines(copy.deepcopy(vio), n_line=9, n_const=2)])
    batch = [synthetic.make_window(seed=1000 + i) for i in range(64)]
    layout("batch64", batch)
    layout("batch64_lm", batch, env={"SADVIO_LM": "1"})
    layout("contig", [c2], env={"SADVIO_CONTIG_TILES": "1"})
    layout("update", [add_lines(copy.deepcopy(ws), n_line=5, n_const=1)], one_build=True)
    c4 = synthetic.make_window(n_kf=100, n_lmk=50000, length=50.0, band=6, seed=4)
    layout("shard1of4", [sharding.shard_window(c4, 1, 4)], before=lambda be: be.set_collective(1, 4, lambda ctx, ptr, count, stream: 0))


def run(lib):
    env = dict(os.environ, SADVIO_BA_LIB=os.path.abspath(lib), SADVIO_DEBUG="8192")
    p = subprocess.run([sys.executable, os.path.abspath(__file__), "--child"], env=env, capture_output=True, text=True, timeout=900)
    if p.returncode != 0:
        print(f"{lib}: the child ended with status {p.returncode}; nothing further is started\n{p.stderr[-2000:]}")
        sys.exit(3)
    layouts, name = collections.OrderedDict(), None
    for ln in p.stderr.splitlines():
        if ln.startswith("== layout "): name = ln[10:]; layouts[name] = collections.Counter()
        elif ln.startswith("[sadvio dbg]") and not ln.endswith(" ms") and name: layouts[name][ln] += 1
    return layouts


def main(old_lib, new_lib):
    old = run(old_lib)
    new = run(new_lib)
    ok = list(old) == list(new)
    for name in old:
        a, b = old[name], new.get(name, collections.Counter())
        n_up = sum(v for k, v in a.items() if " upload " in k); n_sc = sum(v for k, v in a.items() if " layout scalars " in k)
        same = a == b and n_up > 0 and n_sc > 0
        ok = ok and same
        print(f"{name}: {n_up} uploaded items, {n_sc} scalar lines, {sum(a.values())} lines in all: " + ("equal" if same else "DIFFERENT"))
        for ln in sorted((a - b).elements()): print("  old only:", ln)
        for ln in sorted((b - a).elements()): print("  new only:", ln)
    print("SAME" if ok else "DIFFERENT")
    return 0 if ok else 1


if __name__ == "__main__":
    if sys.argv[1] == "--child":
        child()
    else:
        sys.exit(main(sys.argv[1], sys.argv[2]))
