"""Generator of tests/golden/long_cov_ref.npz: the 50-digit covariance blocks (cov_helpers.mp_blocks) of the windows of
tests/long_cov_helpers.GOLDEN_WINDOWS at the oracle's solution — every key-frame block, the far cross pair, every landmark block, the
50-digit residual |H X - I| and the diagonal of the float64 information matrix they belong to (the test refuses a fixture made for
another matrix); for the windows of CROSS_WINDOWS among them also the rows of the 50-digit inverse that the cross candidates of the
newest free key-frame read (cov_cross_helpers.mp_inverse_for). CPU only, about two minutes in all:

  python scripts/gen_long_cov_golden.py            writes the fixture
  python scripts/gen_long_cov_golden.py --measure  prints n, lambda_min and the yardstick (route a, route b) of EVERY window instead
"""
import argparse
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]

import cov_cross_helpers as xh    # noqa: E402
import cov_helpers as ch          # noqa: E402
import long_cov_helpers as lc     # noqa: E402
from oracle import oracle         # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--measure", action="store_true")
    ap.add_argument("--windows", default="")
    a = ap.parse_args()
    oracle.build()
    if a.measure:
        for name in (a.windows.split(",") if a.windows else [c.name for c in lc.CASES]):
            t0 = time.time()
            info = lc.oracle_information(name, oracle)
            e_a, e_b, res = lc.yardstick(name, info, fresh=not os.path.exists(lc.GOLDEN))
            print(f"{name}: n {info.n} lambda_min {np.linalg.eigvalsh(info.H)[0]:.2e} route a {e_a:.3e} route b {e_b:.3e} residual {res:.1e} ({time.time() - t0:.0f} s)", flush=True)
        return
    out = {}
    for name in lc.GOLDEN_WINDOWS:
        t0 = time.time()
        info = lc.oracle_information(name, oracle)
        mp, res = ch.mp_blocks(info, want_residual=True)
        i, j = lc.far_pair(info.w)
        out.update({f"{name}/kf": mp["kf"], f"{name}/lmk": mp["lmk"], f"{name}/far": mp["cross"](i, j), f"{name}/residual": np.float64(res),
                    f"{name}/H_diag": np.diag(info.H).copy()})
        if name in lc.CROSS_WINDOWS:   # the rows of the 50-digit inverse that the cross candidates of the newest free key-frame read
            X50 = xh.mp_inverse_for(info, np.arange(info.w.n_lmk))
            out[f"{name}/xrows"] = X50[info.kf_idx[lc.free_kfs(info.w)[0]][:6]].copy()
        print(f"{name}: n {info.n}, residual {res:.1e} ({time.time() - t0:.0f} s)", flush=True)
    np.savez_compressed(lc.GOLDEN, **out)
    print(f"wrote {lc.GOLDEN}: {os.path.getsize(lc.GOLDEN)} bytes")


if __name__ == "__main__":
    main()
