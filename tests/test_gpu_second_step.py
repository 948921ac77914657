"""The SECOND LM step against the twin's 50-digit LM loop (tests/step_helpers.py, tests/golden/second_step_ref.npz).

A one-iteration solve never reads what the candidate pass of a step leaves for the next step's linearisation: the pose tables at the
accepted state, and on the throughput path the records that k_lm_pass's candidate pass writes per tile and sub-block slot for the
next k_build_obs (the buffer of ADVICE r05). That hand-over runs on every step after the first; the whole-solve tests hold it to
1e-6. Here a window is solved with gn_options(1) and with gn_options(2), each on a fresh handle; the difference of the two delta
sets is the second step, held to TOL_FACTOR x max(E_REF2, FLOOR) relative to max |reference second step|, where E_REF2 is the C
oracle's own float64 distance from the same reference (tests/test_step_reference_cpu.py keeps the table honest). Cost, model cost
change and radius of trace row 2 are held to the 50-digit row at max(TOL_FACTOR x the oracle's own distance, 1e-11).

Each window runs on the latency kernels, on the throughput kernels (SADVIO_LM=1) and on the throughput kernels with one three-round
tile (two sub-blocks per tile: lm_ksub = 2). Every run prints its multiples (`SECOND_STEP ...`, run with -s) before it asserts."""
import numpy as np
import pytest

import step_helpers as sh

pytestmark = pytest.mark.gpu

RUNS = [(name, window, tag, env, kernels) for name, window, runs in sh.SECOND_CASES for tag, env, kernels in runs]


def solve(backend_cls, w, opts):
    be = backend_cls(device=0, profile_kernels=True)
    try:
        be.set_windows([w])
        s = be.solve(opts)[0]
        return s, be.get_deltas(0), be.get_trace(0), {k: v["launches"] for k, v in be.kernel_times().items()}
    finally:
        be.close()


@pytest.mark.parametrize("name,window,tag,env,kernels", RUNS, ids=[f"{r[0]}-{r[2]}" for r in RUNS])
def test_second_step_against_50_digits(backend_cls, monkeypatch, name, window, tag, env, kernels):
    for k in sh.SWITCHES:
        monkeypatch.delenv(k, raising=False)
    for k, v in env.items():
        monkeypatch.setenv(k, v)
    case = sh.window_case(window)
    w = sh.case_window(case)
    s1, d1, _, _ = solve(backend_cls, w, sh.case_options(case, 1))
    s2, d2, tr, n = solve(backend_cls, w, sh.case_options(case, 2))
    ref = sh.second_reference(window)
    e = sh.step_error(sh.second_step(d1, d2), ref, w)
    e_row = sh.row_error(tr[2], ref["row"]) if len(tr) > 2 else np.inf
    rec = sh.E_REF2[window]
    unit = [max(v, sh.FLOOR) for v in rec[:2]]
    bar_p, bar_l, bar_row = sh.bars2(window)
    print(f"SECOND_STEP {name} {tag} e_ref2 {rec[0]:.1e} {rec[1]:.1e} multiple pose {e[0] / unit[0]:.2f} lmk {e[1] / unit[1]:.2f} "
          f"row {e_row:.1e} (bar {bar_row:.1e}) steps {s1.num_successful_steps} {s2.num_successful_steps}")
    if kernels == "throughput":     # two steps: one opening pass, then the candidate pass of step 1 feeds step 2
        assert (n.get("k_lm_pass0"), n.get("k_build_obs"), n.get("k_lm_pass")) == (1, 2, 2) and "k_build" not in n, n
    else:
        assert n.get("k_build") == 2 and n.get("k_backsub") == 2 and "k_lm_pass" not in n, n
    assert (s1.num_successful_steps, s2.num_successful_steps) == (1, 2)      # the oracle accepts both (test_step_reference_cpu.py)
    assert e[0] <= bar_p, ("pose part", e[0], bar_p)
    assert e[1] <= bar_l, ("landmark part", e[1], bar_l)
    assert e_row <= bar_row, ("trace row 2", e_row, bar_row)
