"""Wall time of the first solve after set_windows on a use_graph handle (the path where the graph key is built and compared).
replay: the same config-2 window is set again, the plan is unchanged, the captured graph is replayed.
recapture: two windows of different tile counts alternate, the plan differs, the graph is captured again.
Usage: SADVIO_BA_LIB=path/to/libsadvio_ba.so python scripts/gpu_time_first_solve.py LABEL
Prints two lines: label, median and min..max over REPS first solves, microseconds."""
import os
import statistics
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from sadvio_amd import capi, synthetic

REPS = 40
label = sys.argv[1]
a = synthetic.make_window(seed=20250404)                      # config 2: 20 KF x 8000 landmarks
b = synthetic.make_window(n_kf=8, n_lmk=900, seed=77)
opts = capi.gn_options(10)
be = capi.Backend(device=0, use_graph=True)


def first_solve(w):
    be.set_windows([w])
    t0 = time.perf_counter()
    be.solve(opts)
    return (time.perf_counter() - t0) * 1e6


for w in (a, b, a, b):   # warm: allocations, code objects
    first_solve(w)
first_solve(a)
replay = [first_solve(a) for _ in range(REPS)]
recap = []
for _ in range(REPS):
    first_solve(b)
    recap.append(first_solve(a))
be.close()
for name, v in (("replay", replay), ("recapture", recap)):
    print(f"{label} first solve, {name}: median {statistics.median(v):.1f} us (min {min(v):.1f}, max {max(v):.1f}, {REPS} solves)", flush=True)
