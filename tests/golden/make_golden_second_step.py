"""Writes tests/golden/second_step_ref.npz: the 50-digit SECOND LM step of the windows step_helpers.SECOND_WINDOWS, from the twin's own
LM loop (oracle/twin.py::lm_solve, kind="mp", use_schur=True) at 1 and at 2 iterations, differenced before the rounding to float64.
Keys "<window>/<field>" with the fields pose [n_kf, 6], lmk [n_lmk, 3] (the second step) and row [8] (row 2 of the twin's trace: cost,
cost change, radius, step norm, relative decrease, successful, gradient max, model cost change). Nothing here reads the C oracle.

    python tests/golden/make_golden_second_step.py      (a few minutes: four 50-digit solves side by side)"""
import multiprocessing as mp
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))


def one(job):
    import step_helpers as sh
    window, iters = job
    x, log = sh.mp_lm_state(window, iters)
    return window, iters, x, log


def main():
    import step_helpers as sh
    jobs = [(w, it) for w in sh.SECOND_WINDOWS for it in (2, 1)]
    got = {}
    with mp.Pool(min(8, len(jobs))) as pool:
        for window, iters, x, log in pool.imap_unordered(one, jobs):
            got[window, iters] = (x, log)
            print(window, iters, "iterations: cost", log[-1][0], flush=True)
    out = {}
    for window in sh.SECOND_WINDOWS:
        (x1, log1), (x2, log2) = got[window, 1], got[window, 2]
        assert np.array_equal(log1[1], log2[1])          # the same first step
        for k, v in sh.mp_second_step(window, x1, x2, log2).items():
            out[f"{window}/{k}"] = np.asarray(v, dtype=np.float64)
    np.savez(sh.SECOND_GOLDEN, **out)


if __name__ == "__main__":
    main()
