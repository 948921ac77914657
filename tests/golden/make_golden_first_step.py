"""Writes tests/golden/first_step_ref.npz: the 50-digit first LM step (tests/step_helpers.py::mp_first_step) of every case of
step_helpers.CASES marked `golden`, the ones whose reference costs more than a few seconds of Python. Keys "<window>/<field>" with
the fields pose, dv, dba, dbg [n_kf, .], lmk [n_lmk, 3], model_cost_change, cost (after the step), all float64 rounded from 50
digits. Inputs are the oracle's float64 H_full / g_full of the window, so the file depends on the oracle's build only through
roundings far below the bars it serves (tests/test_step_reference_cpu.py re-measures E_REF against it on every run).

    python tests/golden/make_golden_first_step.py [window ...]      (no argument: every golden window; a few minutes on 8 cores)"""
import multiprocessing as mp
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))


def one(window):
    import step_helpers as sh
    from oracle import oracle
    case = next(c for c in sh.CASES if c.window == window)
    ref = sh.mp_first_step(sh.case_window(case), sh.case_options(case), oracle_lib=oracle)
    return window, ref


def main():
    import step_helpers as sh
    from oracle import oracle
    oracle.build()
    todo = sorted({c.window for c in sh.CASES if c.golden and (len(sys.argv) < 2 or c.window in sys.argv[1:])})
    out = dict(np.load(sh.GOLDEN)) if os.path.exists(sh.GOLDEN) and len(sys.argv) > 1 else {}
    with mp.Pool(min(8, len(todo))) as pool:
        for window, ref in pool.imap_unordered(one, todo):
            for k, v in ref.items():
                if k == "mp":
                    continue
                out[f"{window}/{k}"] = np.asarray(v, dtype=np.float64)
            print(window, "model cost change", ref["model_cost_change"], "cost", ref["cost"], flush=True)
    np.savez(sh.GOLDEN, **out)


if __name__ == "__main__":
    main()
