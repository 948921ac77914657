"""What holding long tracks in the reduced system costs, and what marginalising a window with long tracks costs
(profiles/r22_long_track_priors_time.txt). One MI355X; run every leg in a process of its own:

  python scripts/gpu_measure_long_track_priors.py --window long80 --kept 0,10,100
  python scripts/gpu_measure_long_track_priors.py --window cut64 --marg-only          (SADVIO_BA_LIB = another build: A/B)

Window long80: 100 KF x 50 000 landmarks x 5 observations (length 50 m, band 6, seed 4: the config-4 shape) in which every 50th
landmark is a track of 80 observations (band 20, max_depth 40); cut64: those tracks cut to 64 observations, which is what a caller
had to do before long tracks could be marginalised (the windows of profiles/r21_long_tracks_time.txt). --kept k: a full-rank random
dense prior (test_gpu_prior.random_prior's scaling) keeps the first k long tracks. GN-10 wall per solve over 5 solves after a
warm-up, no graph; kernel classes from a profiling handle, 3 solves. marginalize: the oldest key-frame under the reference's selection
rule (synthetic.pre_marginalize), wall over 5 calls after a warm-up, read-back included."""
import argparse
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT); sys.path.insert(0, os.path.join(ROOT, "tests"))

from sadvio_amd import capi, synthetic   # noqa: E402


def build_window(cut):
    import test_gpu_tile_packing as tp
    kw = dict(n_kf=100, seed=4, length=50.0)
    a = synthetic.make_window(n_lmk=50000, obs_per_lmk=5, band=6, **kw)
    b = synthetic.make_window(n_lmk=1000, obs_per_lmk=80, band=20, max_depth=40.0, **kw)
    assert np.array_equal(a.kf_T_f_w[a.kf_const == 1], b.kf_T_f_w[b.kf_const == 1])
    sel = np.arange(64) if cut else None
    w = tp._assemble(a, [(b, l // 50, sel) if l % 50 == 0 else (a, l, None) for l in range(a.n_lmk)])
    return w, list(range(0, a.n_lmk, 50))


def random_prior(long_, k, rng, scale=3.0):
    n = 3 * k
    return {"J": scale * rng.standard_normal((n, n)) / np.sqrt(n), "r0": 0.5 * rng.standard_normal(n), "kf_keep": -1, "kf_col": 0,
            "lmk_index": np.array(long_[:k], dtype=np.int32), "lmk_col": (3 * np.arange(k)).astype(np.int32)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--window", choices=["long80", "cut64"], default="long80")
    ap.add_argument("--kept", default="0")
    ap.add_argument("--marg-only", action="store_true")
    a = ap.parse_args()
    w, long_ = build_window(a.window == "cut64")
    n = np.diff(w.lmk_obs_ptr)
    flags = dict(long_tracks=True, long_track_priors=True) if a.window == "long80" else {}
    tag = os.environ.get("SADVIO_BA_LIB", "this build")
    print(f"{tag}: window {a.window}: {w.n_kf} KF, {w.n_lmk} landmarks, {w.n_obs} observations, {(n > 64).sum()} landmarks above 64 observations (max {n.max()})", flush=True)
    kf0 = w.n_kf - 1
    keep, marg = synthetic.pre_marginalize(w, kf0)
    be = capi.Backend(device=0, **flags)
    be.set_windows([w])
    be.marginalize(0, kf0, marg, keep)
    t = time.perf_counter()
    for _ in range(5):
        g = be.marginalize(0, kf0, marg, keep)
    ms = (time.perf_counter() - t) / 5 * 1e3
    be.close()
    print(f"{tag}:   marginalize key-frame {kf0}: keeps {len(keep)} landmarks ({len(set(keep) & set(long_))} of the 1 000), marginalises {len(marg)}; "
          f"n {g['n']} n_full {g['n_full']}; {ms:.2f} ms per call", flush=True)
    if a.marg_only:
        return
    opts = capi.gn_options(10)
    for k in (int(v) for v in a.kept.split(",")):
        import dataclasses
        wk = w if k == 0 else dataclasses.replace(w, dense_prior=random_prior(long_, k, np.random.default_rng(7)), _keep=[])
        be = capi.Backend(device=0, **flags)
        be.set_windows([wk])
        be.solve(opts)
        t = time.perf_counter()
        for _ in range(5):
            s = be.solve(opts)[0]
        ms = (time.perf_counter() - t) / 5 * 1e3
        be.close()
        be = capi.Backend(device=0, profile_kernels=True, **flags)
        be.set_windows([wk])
        for _ in range(3):
            be.solve(opts)
        kt = be.kernel_times()
        be.close()
        print(f"{tag}:   {k} long tracks kept: GN-10 solve {ms:.2f} ms wall; cost {s.initial_cost:.6g} -> {s.final_cost:.6g}, {s.num_successful_steps} accepted steps", flush=True)
        print(f"{tag}:     kernel classes, us per launch: " + ", ".join(f"{c} {v['avg_us']:.1f} (x{v['launches']})" for c, v in kt.items()), flush=True)


if __name__ == "__main__":
    main()
