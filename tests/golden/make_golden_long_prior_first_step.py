"""Writes tests/golden/long_prior_first_step_ref.npz: the 50-digit first LM step (tests/step_helpers.py: mp_first_step) of every window
of tests/long_prior_helpers.py under the prior that keeps its long tracks, rounded to float64.
Run from the repository root: python tests/golden/make_golden_long_prior_first_step.py"""
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE)); sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))

import long_prior_helpers as ph   # noqa: E402
from oracle import oracle         # noqa: E402

if __name__ == "__main__":
    oracle.build()
    out = {}
    for c in ph.CASES:
        ref = ph.reference(c, oracle, fresh=True)
        for k in ("pose", "dv", "dba", "dbg", "lmk"):
            out[f"{c.window}/{k}"] = ref[k]
        out[f"{c.window}/model_cost_change"] = np.float64(ref["model_cost_change"])
        out[f"{c.window}/cost"] = np.float64(ref["cost"])
        print(c.window, ref["model_cost_change"], ref["cost"], flush=True)
    np.savez_compressed(ph.GOLDEN, **out)
