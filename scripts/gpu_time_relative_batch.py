#!/usr/bin/env python
"""Time of sadvio_ba_marginalize_relative_batch against the loop of sadvio_ba_marginalize_relative calls it replaces.

  python scripts/gpu_time_relative_batch.py [OUT.txt]

The window of the config-5 test (tests/test_gpu_relative.py): 500 KF x 40 000 landmarks, band = 6, pairs (k, k + 1) and (k, k + 2).
For the first 16, the first 128 and all pairs: wall time of one batch call (median of 5, after a warm-up call that builds the
per-key-frame landmark lists and grows the work buffers), wall time of the loop of single-pair calls over the same pairs on the same
handle (one pass, after a warm-up of 16 calls), and the device time of k_rel_batch between hipEvents on a second handle created with
cfg.profile_kernels. The lines are printed and, with OUT.txt, written there (meant for profiles/r11_relative_batch_time.txt).
"""
import os, sys, time
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import numpy as np


def main(out_path):
    from sadvio_amd import capi, synthetic
    lines = []

    def say(s):
        print(s, flush=True)
        lines.append(s)

    w = synthetic.make_window(n_kf=500, n_lmk=40000, length=250.0, band=6, seed=5, pixel_noise=0.5)
    pairs_all = [(k, k + s) for k in range(w.n_kf - 1) for s in (1, 2) if k + s < w.n_kf]
    say(f"window: {w.n_kf} KF, {w.n_lmk} landmarks, {w.n_obs} observations, band 6; {len(pairs_all)} pairs (k, k + 1), (k, k + 2)")
    be = capi.Backend(device=0)
    bp = capi.Backend(device=0, profile_kernels=True)
    be.set_windows([w]); bp.set_windows([w])
    be.marginalize_relative_batch(0, pairs_all[:16])
    for a, b in pairs_all[:16]:
        be.marginalize_relative(0, a, b)
    for n in (16, 128, len(pairs_all)):
        pairs = pairs_all[:n]
        be.marginalize_relative_batch(0, pairs)
        walls = []
        for _ in range(5):
            t = time.perf_counter()
            got = be.marginalize_relative_batch(0, pairs)
            walls.append(time.perf_counter() - t)
        t = time.perf_counter()
        single = [be.marginalize_relative(0, a, b) for a, b in pairs]
        loop = time.perf_counter() - t
        n_ok = int((got["status"] == capi.SADVIO_OK).sum())
        assert [s is not None for s in single] == [bool(x) for x in got["status"] == capi.SADVIO_OK]
        worst = max(np.abs(s[1] - got["Ak"][i]).max() / np.abs(s[1]).max() for i, s in enumerate(single) if s is not None)
        k0 = bp.kernel_times().get("k_rel_batch", {"avg_us": 0.0, "launches": 0})
        for _ in range(5):
            bp.marginalize_relative_batch(0, pairs)
        k1 = bp.kernel_times()["k_rel_batch"]
        dev = (k1["avg_us"] * k1["launches"] - k0["avg_us"] * k0["launches"]) / (k1["launches"] - k0["launches"])
        batch = float(np.median(walls))
        say(f"{n:4d} pairs ({n_ok} OK, shared landmarks {got['n_shared'].min()} .. {got['n_shared'].max()}): batch call {batch * 1e3:9.3f} ms wall "
            f"(k_rel_batch {dev / 1e3:.3f} ms on the device), loop of single-pair calls {loop * 1e3:9.1f} ms wall, "
            f"{loop / batch:.0f} x; max |Ak_batch - Ak_single| / max|Ak| {worst:.1e}")
    be.close(); bp.close()
    if out_path:
        with open(out_path, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main(sys.argv[1] if len(sys.argv) > 1 else None)
