"""k_solve<0, .> with the first pivot block started as soon as tile (0, 0) is ready and the finalisation test run under the first panel
(kernels.h: SolveEndHook; chol16.h: c16_solve_hooked), and with the back-substitution of chol16.h in its new order.

  * The first LM step of N_p = 6, 18, 48, 96, 114, 174 (the windows of tests/test_gpu_solve_tail_sizes.py, at most 350 observations)
    against the 50-digit first step at the bar of step_helpers; N_p = 114 on a graph handle as well.
  * The same step from a library built with -DSADVIO_C16_PARENT_ORDER, loaded through SADVIO_BA_LIB in a child process (the library path
    is read when sadvio_amd.capi is imported). The macro changes no floating-point operation (tests/test_gpu_chol16_order.py proves that
    on the same image), but k_build's sums over several tiles are not bit-reproducible: the one-wave N_p = 18 window must come out bit
    for bit, the others as two runs of one build do — within twice the largest difference between 8 default runs.
  * Solves that END inside k_solve, at N_p = 6 (one block column) and N_p = 114 (eight; the verdict is read at the barrier in front of
    the back-substitution), on a graph-less and, for N_p = 114, a graph handle: a gradient tolerance
    above the initial gradient (slot 0: no step, deltas zero), one between the gradient maxima of two consecutive iterations of an
    unconstrained run (read from its trace), and max_num_iterations = 0. Termination, iterations, costs and deltas against the oracle's
    solve of the same window and options, at the bars of tests/test_gpu_edges.py (the library against the oracle after several steps).
  * Two windows of different N_p in one submission, one ending at slot 0 while the other runs on: each equals its single-window result
    (the ended one exactly; the other as two runs of one build do).
  * k_solve<0, true>: the smallest IMU window of step_helpers (dpf = 15), first step at its bar and one ended solve.

Every case prints its figures (`SOLVE_CHAIN ...`, run with -s) before it asserts."""
import itertools
import os
import shutil
import subprocess
import sys

import numpy as np
import pytest

import __graft_entry__ as ge
import step_helpers as sh
import test_gpu_edges as edges
import test_gpu_first_step as first
import test_gpu_solve_tail_sizes as tails
from sadvio_amd import capi

pytestmark = pytest.mark.gpu

NP = (6, 18, 48, 96, 114, 174)
CASES = [c for c in tails.CASES if c.np_ in NP]
CASE = {c.np_: c for c in CASES}
MACRO = "-DSADVIO_C16_PARENT_ORDER"
DEFAULT_RUNS = tails.DEFAULT_RUNS
UNCONSTRAINED = 6          # iterations of the run whose trace gives the gradient maxima
VIO = sh.CASE["vio15"]     # the smallest IMU window: two key-frames, one of them free, 15 states


def solve(backend_cls, windows, opts, graph=False):
    """[(summary, deltas, trace)] of one solve of the windows on a fresh handle."""
    be = backend_cls(device=0, use_graph=graph)
    try:
        be.set_windows(list(windows))
        sums = be.solve(opts)
        return [(sums[i], be.get_deltas(i), be.get_trace(i)) for i in range(len(windows))]
    finally:
        be.close()


def clear_switches(monkeypatch):
    for k in sh.SWITCHES + (tails.SWITCH,):
        monkeypatch.delenv(k, raising=False)


def distance(a, b):
    return max(float(np.abs(a[k] - b[k]).max()) for k in ("pose", "lmk"))


def test_the_windows_are_the_sizes_of_the_issue():
    assert tuple(c.np_ for c in CASES) == NP
    for c in CASES:
        w = sh.case_window(c)
        assert sh.layout(w)["Nr"] == c.np_ and len(w.obs_kf) <= tails.MAX_OBS
    assert sh.layout(sh.case_window(VIO))["dpf"] == 15 and sh.layout(sh.case_window(VIO))["Nr"] == 15


@pytest.mark.parametrize("np_, graph", [(n, False) for n in NP] + [(114, True)])
def test_first_step_against_50_digits(backend_cls, oracle_lib, monkeypatch, np_, graph):
    clear_switches(monkeypatch)
    case = CASE[np_]
    w = sh.case_window(case)
    ref, e_ref = tails.reference(case, oracle_lib)
    s, d, tr = solve(backend_cls, [w], sh.case_options(case), graph)[0]
    e = sh.step_error(d, ref, w)
    unit = [max(v, sh.FLOOR) for v in e_ref]
    print(f"SOLVE_CHAIN first step Np {np_} graph {int(graph)} e_ref {e_ref[0]:.1e} {e_ref[1]:.1e} multiple pose {e[0] / unit[0]:.2f} lmk {e[1] / unit[1]:.2f} "
          f"steps {s.num_successful_steps}")
    assert s.num_successful_steps == 1
    assert e[0] <= sh.TOL_FACTOR * unit[0], ("pose part", e[0], sh.TOL_FACTOR * unit[0])
    assert e[1] <= sh.TOL_FACTOR * unit[1], ("landmark part", e[1], sh.TOL_FACTOR * unit[1])
    assert np.isclose(tr[1][7], ref["model_cost_change"], rtol=1e-11, atol=0)


# ---- the same step from a build with the parent's instruction order -------------------------------------------------------------------
CHILD = """
import sys
sys.path[:0] = [{root!r}, {tests!r}]
import numpy as np
import step_helpers as sh
import test_gpu_solve_tail_sizes as tails
from sadvio_amd import capi
assert capi.LIB_PATH == {lib!r}, capi.LIB_PATH
capi.load_library()
out = {{}}
for c in tails.CASES:
    if c.np_ not in {nps!r}:
        continue
    be = capi.Backend(device=0)
    be.set_windows([sh.case_window(c)])
    s = be.solve(sh.case_options(c))[0]
    d = be.get_deltas(0)
    be.close()
    assert s.num_successful_steps == 1
    out[f"{{c.np_}}/pose"], out[f"{{c.np_}}/lmk"] = d["pose"], d["lmk"]
np.savez({out!r}, **out)
"""


@pytest.fixture(scope="module")
def parent_order_steps(tmp_path_factory):
    """{N_p: deltas of the first step} from a library built with the macro, solved in one child process."""
    hipcc = shutil.which("hipcc") or next((p for p in ("/opt/rocm/bin/hipcc",) if os.access(p, os.X_OK)), None)
    if hipcc is None:
        pytest.skip("no hipcc on this machine: the library with " + MACRO + " was not built")
    tmp = tmp_path_factory.mktemp("parent_order")
    lib, out = str(tmp / "libsadvio_ba_parent_order.so"), str(tmp / "steps.npz")
    subprocess.run([hipcc] + ge.HIP_FLAGS + [MACRO, "-o", lib] + [os.path.join(ge.CSRC, s) for s in ge.HIP_SOURCES], check=True, cwd=ge.CSRC, timeout=900)
    env = {k: v for k, v in os.environ.items() if k not in sh.SWITCHES + (tails.SWITCH,)}
    env["SADVIO_BA_LIB"] = lib
    code = CHILD.format(root=ge.ROOT, tests=os.path.dirname(os.path.abspath(__file__)), lib=lib, nps=NP, out=out)
    r = subprocess.run([sys.executable, "-c", code], env=env, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, (r.stdout + r.stderr)[-3000:]
    z = np.load(out)
    return {n: {"pose": z[f"{n}/pose"], "lmk": z[f"{n}/lmk"]} for n in NP}


@pytest.mark.parametrize("np_", NP)
def test_parent_order_build_agrees_as_two_runs_do(backend_cls, monkeypatch, parent_order_steps, np_):
    clear_switches(monkeypatch)
    case = CASE[np_]
    new = [solve(backend_cls, [sh.case_window(case)], sh.case_options(case))[0][1] for _ in range(DEFAULT_RUNS)]
    old = parent_order_steps[np_]
    spread = max(distance(a, b) for a, b in itertools.combinations(new, 2))
    dist = distance(new[0], old)
    print(f"SOLVE_CHAIN Np {np_} parent-order build against this one: max |difference| {dist:.3e}, between {DEFAULT_RUNS} default runs {spread:.3e}"
          + (" (one wave of one tile: bit equality)" if np_ == 18 else ""))
    if np_ == 18:
        assert all(np.array_equal(new[0][k], old[k]) for k in ("pose", "lmk"))
    assert dist <= 2.0 * spread


# ---- solves that end inside k_solve ----------------------------------------------------------------------------------------------------
_gmax = {}


def gradient_maxima(backend_cls, name, w):
    """Gradient maxima at the states of an unconstrained run of UNCONSTRAINED iterations (column 6 of the trace), once per window."""
    if name not in _gmax:
        tr = solve(backend_cls, [w], capi.gn_options(UNCONSTRAINED))[0][2]
        _gmax[name] = np.array([row[6] for row in tr[:UNCONSTRAINED]])
    return _gmax[name]


def ending_options(backend_cls, name, w, how):
    """(options, slot the solve ends at) of one way to end a solve inside k_solve."""
    if how == "zero_iterations":
        return capi.gn_options(0), 0
    g = gradient_maxima(backend_cls, name, w)
    o = capi.gn_options(UNCONSTRAINED)
    if how == "slot0":
        o.gradient_tolerance = 2.0 * g[0]
        return o, 0
    # the first pair of consecutive iterations a factor of 4 apart: the tolerance is their geometric mean, a factor of 2 from either,
    # far outside the last digits in which the oracle's gradient differs from the device's
    j = next(i for i in range(1, len(g)) if 0 < g[i] < 0.25 * g[i - 1])
    o.gradient_tolerance = float(np.sqrt(g[j] * g[j - 1]))
    return o, j


def check_ended(be_result, ref, w, slot, vio=False):
    s, d, tr = be_result
    rs = ref["summary"]
    print(f"SOLVE_CHAIN ended at slot {slot}: iterations {s.iterations} | {rs.iterations} termination {s.termination} | {rs.termination} "
          f"cost {s.initial_cost!r} -> {s.final_cost!r} | {rs.initial_cost!r} -> {rs.final_cost!r} max |pose| {np.abs(d['pose']).max():.3e}")
    assert (s.iterations, s.termination) == (rs.iterations, rs.termination)
    assert s.iterations == slot
    assert (s.num_successful_steps, s.num_unsuccessful_steps) == (rs.num_successful_steps, rs.num_unsuccessful_steps)
    assert np.isclose(s.initial_cost, rs.initial_cost, rtol=1e-9) and np.isclose(s.final_cost, rs.final_cost, rtol=1e-9)
    assert len(tr) == slot + 1
    if slot == 0:      # no step, no candidate: the deltas are zero, not small
        assert all(np.all(d[k] == 0.0) for k in ("pose", "lmk", "dv", "dba", "dbg"))
        assert s.final_cost == s.initial_cost
    assert np.abs(d["pose"] - ref["pose"]).max() <= edges.POSE_TOL
    assert edges.lmk_err(d["lmk"], ref["lmk"]) <= edges.LMK_TOL
    if vio:
        for q in ("dv", "dba", "dbg"):
            assert np.abs(d[q] - ref[q]).max() <= edges.POSE_TOL


@pytest.mark.parametrize("how", ["slot0", "between_iterations", "zero_iterations"])
@pytest.mark.parametrize("np_, graph", [(6, False), (114, False), (114, True)])
def test_ended_solve_equals_the_oracle(backend_cls, oracle_lib, monkeypatch, np_, graph, how):
    clear_switches(monkeypatch)
    w = sh.case_window(CASE[np_])
    opts, slot = ending_options(backend_cls, f"tail{np_}", w, how)
    assert (slot >= 1) == (how == "between_iterations")
    ref = oracle_lib.solve(w, opts)
    check_ended(solve(backend_cls, [w], opts, graph)[0], ref, w, slot)


def test_two_windows_one_ends_at_slot_0_the_other_runs_on(backend_cls, oracle_lib, monkeypatch):
    clear_switches(monkeypatch)
    ws = [sh.case_window(CASE[6]), sh.case_window(CASE[114])]
    g0 = [gradient_maxima(backend_cls, f"tail{n}", w)[0] for n, w in zip((6, 114), ws)]
    lo, hi = (0, 1) if g0[0] < g0[1] else (1, 0)       # the window with the smaller initial gradient ends at slot 0
    assert g0[hi] > 1.5 * g0[lo], g0
    o = capi.gn_options(3)
    o.gradient_tolerance = float(np.sqrt(g0[lo] * g0[hi]))
    both = solve(backend_cls, ws, o)
    singles = [[solve(backend_cls, [w], o)[0] for _ in range(DEFAULT_RUNS if i == hi else 1)] for i, w in enumerate(ws)]
    s, d, tr = both[lo]
    s1, d1, tr1 = singles[lo][0]
    print(f"SOLVE_CHAIN two windows: initial gradients {g0[0]:.3e} {g0[1]:.3e}, tolerance {o.gradient_tolerance:.3e}; window {lo} iterations {s.iterations}, "
          f"window {hi} iterations {both[hi][0].iterations}")
    assert (s.iterations, s.termination, s.initial_cost, s.final_cost) == (0, s1.termination, s1.initial_cost, s1.final_cost) and s1.iterations == 0
    assert all(np.all(d[k] == 0.0) and np.all(d1[k] == 0.0) for k in ("pose", "lmk"))
    s, d, tr = both[hi]
    runs = singles[hi]
    assert s.iterations >= 1 and all((r[0].iterations, r[0].termination, r[0].num_successful_steps) == (s.iterations, s.termination, s.num_successful_steps) for r in runs)
    spread = max(distance(a[1], b[1]) for a, b in itertools.combinations(runs, 2))
    dist = distance(d, runs[0][1])
    print(f"SOLVE_CHAIN two windows: running window against its single-window solve {dist:.3e}, between {DEFAULT_RUNS} single-window runs {spread:.3e}")
    assert dist <= 2.0 * spread
    assert np.isclose(s.final_cost, runs[0][0].final_cost, rtol=1e-12)
    ref = oracle_lib.solve(ws[hi], o)
    assert (s.iterations, s.termination) == (ref["summary"].iterations, ref["summary"].termination)
    assert np.abs(d["pose"] - ref["pose"]).max() <= edges.POSE_TOL


# ---- k_solve<0, true> ------------------------------------------------------------------------------------------------------------------
def test_extras_first_step_against_50_digits(backend_cls, oracle_lib, monkeypatch):
    s, d, tr, kt = first.run_case(backend_cls, monkeypatch, VIO)
    first.check_case(VIO, oracle_lib, s, d, tr, tag=" (solve chain)")


def test_extras_ended_solve_equals_the_oracle(backend_cls, oracle_lib, monkeypatch):
    clear_switches(monkeypatch)
    w = sh.case_window(VIO)
    opts, slot = ending_options(backend_cls, "vio15", w, "slot0")
    ref = oracle_lib.solve(w, opts)
    check_ended(solve(backend_cls, [w], opts)[0], ref, w, slot, vio=True)
