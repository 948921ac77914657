#!/usr/bin/env python
"""How often does a GN-10 solve of tests/test_gpu_parity.py::test_solve_matches_oracle_small land outside its 1e-6 landmark bar?

  python scripts/gpu_repeat_parity.py [SOLVES] [LIB ...]

With early exits disabled the attempts after convergence accept or reject on cost changes of rounding size; on the angular window
the number of accepted steps then varies from run to run and, with it, the weakly observed landmarks by up to 2e-6. Each LIB (a
build of libsadvio_ba.so; default: the tree's) is measured in a process of its own, so two builds can be compared.
"""
import os, subprocess, sys
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT); sys.path.insert(0, os.path.join(ROOT, "tests"))


def child(n):
    import numpy as np
    from golden_util import lmk_err
    from oracle import oracle
    from sadvio_amd import capi, synthetic
    oracle.build()
    for factor in (capi.FACTOR_ANGULAR, capi.FACTOR_PIXEL):
        w = synthetic.make_window(n_kf=6, n_lmk=400, seed=7, factor=factor)
        opts = capi.gn_options(10)
        ref = oracle.solve(w, opts)
        out = []
        for _ in range(n):
            be = capi.Backend(device=0)
            be.set_windows([w]); s = be.solve(opts)[0]; d = be.get_deltas(0); be.close()
            out.append((lmk_err(d["lmk"], ref["lmk"]), float(np.abs(d["pose"] - ref["pose"]).max()), s.num_successful_steps))
        le = np.array([o[0] for o in out])
        print(f"  factor {factor}: {n} solves, landmark error min {le.min():.3e} median {np.median(le):.3e} max {le.max():.3e}, over 1e-6: {(le > 1e-6).sum()}; "
              f"pose max {max(o[1] for o in out):.3e}; successful steps {sorted(set(o[2] for o in out))} (oracle {ref['summary'].num_successful_steps})", flush=True)


if __name__ == "__main__":
    if len(sys.argv) > 2 and sys.argv[1] == "child":
        child(int(sys.argv[2])); sys.exit(0)
    n = int(sys.argv[1]) if len(sys.argv) > 1 else 40
    for lib in (sys.argv[2:] or [None]):
        env = dict(os.environ)
        if lib: env["SADVIO_BA_LIB"] = os.path.abspath(lib)
        print(lib or "the tree's library", flush=True)
        r = subprocess.run([sys.executable, os.path.abspath(__file__), "child", str(n)], env=env, timeout=300)
        if r.returncode != 0: sys.exit(r.returncode)
