"""The block-diagonal / gradient sums of k_build's MFMA tiles (ds_add_f64 from the head lanes into the LDS tile, flushed with the MFMA
accumulators): every wave adds from all of its landmark groups, also when its 8 landmarks list the same key-frames in the same lanes
(those waves used to sum across their groups with DPP first and add from one group).

Every case is solved with reference_options() and with gn_options(10) and checked against the CPU oracle with the bars of
test_gpu_tile_packing (final cost rtol 1e-9, POSE_TOL, LMK_TOL). The windows are the smallest at which a piece of these sums can go
wrong: idle waves, a one-landmark tile beside a full one, a tile whose waves are all uniform (every group adds to the same addresses),
tiles of 1, 2 and 5 free key-frames (one MFMA tile against three), waves whose every lane is a head, several landmark rounds per tile,
runs of up to four lanes on one key-frame, and a tile left in LDS by an earlier launch or layout.

No comparison between two summation orders is made at 1e-10: these windows converge in 3 - 4 steps, the remaining attempts of
gn_options(10) are accepted or rejected on cost changes at rounding level, and the result then depends on the summation order by
itself - the CPU oracle run with 1 against 4 threads differs by up to 2e-7 on them.
"""
import numpy as np
import pytest

from sadvio_amd import capi, synthetic
from sparse_helpers import vio_sparse_priors
from test_gpu_tile_packing import _assemble, _check_against_oracle, _pair, _wide
from vio_helpers import make_vio_window

pytestmark = pytest.mark.gpu

MODES = ["ref", "gn10"]


def _opts(mode):
    return capi.reference_options() if mode == "ref" else capi.gn_options(10)


def _head_overflow():
    """One observation in each of key-frames 1 .. 5 per landmark: 16 such landmarks are two waves of 40 head lanes each (every lane that carries an observation adds); behind them the narrow tracks that stay inside those key-frames."""
    a, b = _pair(8, 200, 400, 11)
    wd = _wide(b, 1, 5)
    assert len(wd) >= 16, len(wd)
    narrow = [(a, l, None) for l in range(a.n_lmk)
              if 1 <= a.obs_kf[a.lmk_obs_ptr[l]:a.lmk_obs_ptr[l + 1]].min() and a.obs_kf[a.lmk_obs_ptr[l]:a.lmk_obs_ptr[l + 1]].max() <= 5]
    assert len(narrow) >= 12, len(narrow)
    return _assemble(a, wd[:16] + narrow[:12])


def _one_landmark():
    a = synthetic.make_window(n_kf=6, n_lmk=8, seed=13)
    return _assemble(a, [(a, 3, None)])


def _vio_rare():
    """A VIO window whose sparse prior holds landmarks: their pseudo-observations sit beside the real ones on the prior's key-frame
    (runs of up to four lanes), the tiles run k_build<RARE, IMU>."""
    w = make_vio_window(n_kf=4, n_lmk=40, seed=67)
    w.sparse_priors = vio_sparse_priors(w, w.n_kf - 2, list(range(0, 20, 2)), np.random.default_rng(6), noise=0.03)
    return w


CASES = {
    "one_landmark": _one_landmark,                                                   # three waves have nothing to add
    "33_landmarks": lambda: synthetic.make_window(n_kf=6, n_lmk=33, seed=31),         # a full tile and a one-landmark tile
    "64_landmarks": lambda: synthetic.make_window(n_kf=6, n_lmk=64, seed=32),         # heads at different lanes per group; one constant key-frame
    "uniform_tile": lambda: synthetic.make_window(n_kf=4, n_lmk=32, obs_per_lmk=8, seed=38),   # all 8 views of every landmark: every wave is uniform
    "1_free_kf": lambda: synthetic.make_window(n_kf=2, n_lmk=40, obs_per_lmk=4, seed=33),   # Nt = 6
    "2_free_kf": lambda: synthetic.make_window(n_kf=3, n_lmk=40, obs_per_lmk=5, seed=34),   # Nt = 12
    "5_free_kf": lambda: synthetic.make_window(n_kf=6, n_lmk=32, obs_per_lmk=8, seed=35),   # Nt = 30: three MFMA tiles
    "head_overflow": _head_overflow,
    "vio_rare": _vio_rare,
}


_WINDOWS = {}


def _window(name):
    """Built once for both option sets (the windows are only read)."""
    if name not in _WINDOWS:
        _WINDOWS[name] = CASES[name]()
    return _WINDOWS[name]


@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("name", list(CASES))
def test_tile_sums_match_oracle(backend_cls, oracle_lib, name, mode):
    _check_against_oracle(backend_cls, oracle_lib, _window(name), mode)


def _solve_batch(backend_cls, ws, opts):
    be = backend_cls(device=0)
    try:
        be.set_windows(ws)
        ss = be.solve(opts)
        return [(ss[i], be.get_deltas(i)) for i in range(len(ws))]
    finally:
        be.close()


@pytest.mark.parametrize("mode", MODES)
def test_two_rounds_add_into_one_tile(backend_cls, oracle_lib, monkeypatch, mode):
    """SADVIO_TILE_ROUNDS=2 on a two-window batch: 64 landmarks per tile, every wave adds two rounds into the tile."""
    from golden_util import lmk_err
    from test_gpu_parity import LMK_TOL, POSE_TOL
    ws = [synthetic.make_window(n_kf=6, n_lmk=100, seed=36), synthetic.make_window(n_kf=5, n_lmk=70, seed=37)]
    opts = _opts(mode)
    monkeypatch.setenv("SADVIO_TILE_ROUNDS", "2")
    new = _solve_batch(backend_cls, ws, opts)
    for w, n in zip(ws, new):
        ref = oracle_lib.solve(w, opts)
        assert np.isclose(n[0].final_cost, ref["summary"].final_cost, rtol=1e-9)
        if mode == "ref":
            assert (n[0].iterations, n[0].termination) == (ref["summary"].iterations, ref["summary"].termination)
        assert np.abs(n[1]["pose"] - ref["pose"]).max() <= POSE_TOL and lmk_err(n[1]["lmk"], ref["lmk"]) <= LMK_TOL


def test_graph_replay_and_a_new_layout_start_from_a_zeroed_tile(backend_cls, oracle_lib):
    """The replay of a captured graph, and then a smaller window on the same handle (fewer waves with landmarks, fewer key-frames), must
    not pick up what an earlier launch left in LDS."""
    from golden_util import lmk_err
    from test_gpu_parity import LMK_TOL, POSE_TOL
    opts = capi.reference_options()
    big, small = synthetic.make_window(n_kf=6, n_lmk=64, seed=32), _one_landmark()

    def run():
        be = backend_cls(device=0, use_graph=True)
        try:
            out = []
            for w in (big, small):
                be.set_windows([w])
                be.solve(opts)
                s = be.solve(opts)[0]          # the replay of the captured graph
                out.append((s, be.get_deltas(0)))
            return out
        finally:
            be.close()
    for w, n in zip((big, small), run()):
        ref = oracle_lib.solve(w, opts)
        assert np.isclose(n[0].final_cost, ref["summary"].final_cost, rtol=1e-9)
        assert np.abs(n[1]["pose"] - ref["pose"]).max() <= POSE_TOL and lmk_err(n[1]["lmk"], ref["lmk"]) <= LMK_TOL
