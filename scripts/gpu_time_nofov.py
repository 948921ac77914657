#!/usr/bin/env python
"""Wall time of sadvio_ba_nofov_scale (the whole NoFov LM solve and its gate in one kernel launch, host tables and copies
included) on a scaleTest-sized problem and on one at the landmark cap."""
import os, sys, time
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
from sadvio_amd import capi
import nofov_helpers as H
be = capi.Backend(device=0)
cases = [("scaleTest (10 000 points)", dict(seed=0, n_points=10000, px_noise=0.2)),
         ("cap (65 536 landmarks, 6 extra key-frames)", dict(seed=8, n_points=400000, px_noise=0.2, lmk_noise=0.02, n_outliers=500,
                                                            n_extra=6, max_lmk=65536))]
for name, kw in cases:
    pb = H.abi(H.make_nofov(**kw))
    for _ in range(3): r = be.nofov_scale(**pb)
    reps = 20
    t = time.perf_counter()
    for _ in range(reps): r = be.nofov_scale(**pb)
    us = (time.perf_counter() - t) / reps * 1e6
    print(f"NoFov {name}: {len(pb['lmk_p'])} landmarks, {len(pb['obs_frame'])} angular factors, {us:.0f} us per call, "
          f"{r['summary'].iterations} iterations, lambda {r['lambda']:.6f}", flush=True)
be.close()
