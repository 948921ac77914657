#!/usr/bin/env python
"""Host-time breakdown of sadvio_ba_set_windows (SADVIO_DEBUG=8192 laps of layout_build and of the planning steps it calls, layout_driver.h / layout_plan.h; with that switch every flush also hashes its payload, so read the laps, not the medians) on the config-2 window and the config-3 shaped
VIO window: python scripts/set_windows_laps.py
Against lap tables from before the planner / driver split: "layout_reduced" is now the host planning of the reduced systems alone and is
printed before "alloc+queue"; their allocations, memsets, the dense priors' flush and the prepare launches are the new lap "reduced
device" (they were part of "layout_reduced"); "chunks" (chunk tables and work lists of the throughput kernels) was part of "alloc+queue";
"  half-bandwidth", which timed nothing, is gone."""
import os, sys, time
os.environ["SADVIO_DEBUG"] = "8192"
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "tests"))
from sadvio_amd import capi, synthetic
from vio_helpers import make_vio_window
for name, w in (("config-2", synthetic.make_window(seed=20250404)), ("config-3 vio", make_vio_window(n_kf=12, n_lmk=7200, seed=6))):
    be = capi.Backend(device=0)
    for _ in range(4): be.set_windows([w])
    ts = []
    for _ in range(20):
        t = time.perf_counter(); be.set_windows([w]); ts.append(time.perf_counter() - t)
    sys.stderr.flush()
    print(f"== {name}: set_windows median {sorted(ts)[10]*1e3:.3f} ms, min {min(ts)*1e3:.3f} ms", file=sys.stderr, flush=True)
    be.close()
