"""Single-window tiles as landmark lists (tile_pack.h): outlier tracks are set aside instead of cutting the run of narrow tracks
around them. The solves are checked against the CPU oracle with the bars of test_gpu_parity.test_solve_matches_oracle_small
(final cost rtol 1e-9, pose / landmark steps 1e-6); the tiling itself is read from the library's SADVIO_DEBUG line in a child
process (the switches are read when a handle is created). SADVIO_CONTIG_TILES forces the contiguous cut.

Windows: narrow tracks (5 observations over 2-3 key-frames) come from synthetic.make_window; outlier tracks are landmarks of a second
window of the same seed (same true poses, so their measurements are consistent) made with 12 observations each, thinned to one
observation per key-frame: 5-6 key-frames wide, so that a tile holding them and their neighbours would touch more than the 5 free
key-frames of the MFMA path.
"""
import os
import re
import subprocess
import sys

import numpy as np
import pytest

from golden_util import lmk_err
from sadvio_amd import capi, synthetic
from test_gpu_parity import LMK_TOL, POSE_TOL

pytestmark = pytest.mark.gpu

TESTS = os.path.dirname(os.path.abspath(__file__))


def _assemble(base, picks):
    """A window with base's key-frames and cameras whose landmarks are picks: (window, landmark, observation positions or None)."""
    lmk_p, ptr, kf, cam, meas = [], [0], [], [], []
    for src, l, sel in picks:
        o = np.arange(src.lmk_obs_ptr[l], src.lmk_obs_ptr[l + 1])
        if sel is not None:
            o = o[sel]
        lmk_p.append(src.lmk_p[l]); kf.append(src.obs_kf[o]); cam.append(src.obs_cam[o]); meas.append(src.obs_meas[o])
        ptr.append(ptr[-1] + len(o))
    return capi.FlatWindow(
        kf_T_f_w=base.kf_T_f_w, kf_const=base.kf_const, cam_K=base.cam_K, cam_T_s_f=base.cam_T_s_f, cam_sigma=base.cam_sigma,
        lmk_p=np.array(lmk_p), lmk_obs_ptr=np.array(ptr, dtype=np.int32), obs_kf=np.concatenate(kf).astype(np.int32),
        obs_cam=np.concatenate(cam).astype(np.int32), obs_meas=np.concatenate(meas), factor_type=base.factor_type, has_imu=0,
        kf_id=base.kf_id, lmk_id=(500000 + 7 * np.arange(len(picks))).astype(np.int64), pose_priors=list(base.pose_priors))


def _one_per_kf(w, l, n):
    """Positions of the first observation of each of the landmark's first n key-frames."""
    k = w.obs_kf[w.lmk_obs_ptr[l]:w.lmk_obs_ptr[l + 1]]
    first = [i for i in range(len(k)) if i == 0 or k[i] != k[i - 1]]
    assert len(first) >= n, (l, k)
    return np.array(first[:n])


def _pair(n_kf, n_narrow, n_wide, seed):
    a = synthetic.make_window(n_kf=n_kf, n_lmk=n_narrow, seed=seed)
    b = synthetic.make_window(n_kf=n_kf, n_lmk=n_wide, obs_per_lmk=12, seed=seed)
    assert np.array_equal(a.kf_T_f_w[a.kf_const == 1], b.kf_T_f_w[b.kf_const == 1])   # same trajectory
    return a, b


def _wide(b, lo, hi, n=5):
    """(landmark, positions) of b's landmarks whose first n key-frames (one observation each) all lie in lo .. hi."""
    out = []
    for j in range(b.n_lmk):
        k = b.obs_kf[b.lmk_obs_ptr[j]:b.lmk_obs_ptr[j + 1]]
        if len(set(k.tolist())) < n: continue
        sel = _one_per_kf(b, j, n)
        if lo <= k[sel].min() and k[sel].max() <= hi: out.append((b, j, sel))
    return out


def _insert(a, at):
    """a's landmarks in order, with the picks at[l] in front of landmark l."""
    picks = []
    for l in range(a.n_lmk):
        picks += at.get(l, [])
        picks.append((a, l, None))
    return _assemble(a, picks)


def make_case(name):
    if name == "outliers":       # 96 narrow tracks over 8 key-frames (newest first); 5 tracks over key-frames 1 .. 5 sit
        a, b = _pair(8, 96, 96, 11)   # between the tracks of the newest ones (two of them adjacent): 6 free key-frames together
        wd = _wide(b, 1, 5)
        assert len(wd) >= 5
        return _insert(a, {10: wd[0:1], 20: wd[1:2], 40: wd[2:4], 50: wd[4:5]})
    if name == "all_outliers":
        a, b = _pair(8, 8, 40, 12)
        return _assemble(a, [(b, j, _one_per_kf(b, j, 6)) for j in range(b.n_lmk)])
    if name == "single":
        a = synthetic.make_window(n_kf=6, n_lmk=8, seed=13)
        return _assemble(a, [(a, 3, None)])
    if name == "g16":            # a 9-observation landmark (16 lanes per landmark) right behind two set-aside ones
        a, b = _pair(8, 64, 96, 11)
        wd = _wide(b, 1, 5)
        assert len(wd) >= 2
        return _insert(a, {5: wd[0:2] + [(b, 0, np.arange(9))]})
    if name == "disjoint":       # two outliers at opposite ends of a 14 key-frame window: no key-frame in common, a tile each
        a, b = _pair(14, 64, 96, 15)
        old, new = _wide(b, 1, 5), _wide(b, 8, 12)
        assert old and new
        return _insert(a, {5: old[0:1], 58: new[0:1]})
    raise KeyError(name)


def _solve(backend_cls, w, opts, use_graph=False):
    be = backend_cls(device=0, use_graph=use_graph)
    try:
        be.set_windows([w])
        s = be.solve(opts)[0]
        if use_graph:
            s = be.solve(opts)[0]    # the replay of the captured graph
        return s, be.get_deltas(0)
    finally:
        be.close()


def _check_against_oracle(backend_cls, oracle_lib, w, mode, use_graph=False):
    opts = capi.reference_options() if mode == "ref" else capi.gn_options(10)
    s, d = _solve(backend_cls, w, opts, use_graph)
    ref = oracle_lib.solve(w, opts)
    rs = ref["summary"]
    assert np.isclose(s.final_cost, rs.final_cost, rtol=1e-9)
    if mode == "ref":
        assert (s.iterations, s.termination) == (rs.iterations, rs.termination)
        assert (s.num_successful_steps, s.num_unsuccessful_steps) == (rs.num_successful_steps, rs.num_unsuccessful_steps)
    assert np.abs(d["pose"] - ref["pose"]).max() <= POSE_TOL and lmk_err(d["lmk"], ref["lmk"]) <= LMK_TOL
    return s, d


@pytest.mark.parametrize("use_graph", [False, True])
@pytest.mark.parametrize("mode", ["ref", "gn10"])
def test_outlier_window_matches_oracle(backend_cls, oracle_lib, mode, use_graph):
    _check_against_oracle(backend_cls, oracle_lib, make_case("outliers"), mode, use_graph)


@pytest.mark.parametrize("name", ["all_outliers", "single", "g16", "disjoint"])
def test_degenerate_windows_match_oracle(backend_cls, oracle_lib, name):
    w = make_case(name)
    _check_against_oracle(backend_cls, oracle_lib, w, "ref")
    _check_against_oracle(backend_cls, oracle_lib, w, "gn10", use_graph=True)


def test_no_packet_route_gives_the_same_result(backend_cls, monkeypatch):
    w = make_case("outliers")
    opts = capi.gn_options(10)
    s0, d0 = _solve(backend_cls, w, opts)
    monkeypatch.setenv("SADVIO_NO_PRE", "1")     # read when the handle is created
    s1, d1 = _solve(backend_cls, w, opts)
    rel = lambda a, b: np.abs(a - b).max() / np.abs(b).max()
    assert abs(s1.final_cost - s0.final_cost) <= 1e-10 * abs(s0.final_cost)
    assert rel(d1["pose"], d0["pose"]) <= 1e-10 and rel(d1["lmk"], d0["lmk"]) <= 1e-10


_CHILD = r"""
import os, sys
sys.path.insert(0, sys.argv[1]); sys.path.insert(0, os.path.dirname(sys.argv[1]))
from sadvio_amd import capi, synthetic
import test_gpu_tile_packing as T
case = sys.argv[2]
for contig in (False, True):
    if contig: os.environ["SADVIO_CONTIG_TILES"] = "1"
    be = capi.Backend(device=0)
    if case == "sharded":
        be.comm_init_rccl(0, 1, be.rccl_unique_id())
    ws = [T.make_case("outliers")]
    if case == "two_windows": ws.append(T.make_case("g16"))
    be.set_windows(ws)
    be.close()
"""


def _tile_lines(case, env=None):
    """The "N tiles, modes ..." line of the packed and of the forced-contiguous layout of a case: (tiles, (global, atomic, gemm), histogram)."""
    e = dict(os.environ, SADVIO_DEBUG="1", **(env or {}))
    e.pop("SADVIO_CONTIG_TILES", None)
    p = subprocess.run([sys.executable, "-c", _CHILD, TESTS, case], env=e, capture_output=True, text=True, timeout=120)
    assert p.returncode == 0, p.stderr[-2000:]
    out = [(int(m.group(1)), tuple(int(m.group(i)) for i in (2, 3, 4)), m.group(5).strip())
           for m in re.finditer(r"(\d+) tiles, modes global/atomic/gemm = (\d+)/(\d+)/(\d+), max_tile_kf \d+, n_free histogram:(.*)", p.stderr)]
    assert len(out) == 2, p.stderr[-2000:]
    return out


def test_packing_saves_tiles_and_keeps_them_in_lds():
    packed, contig = _tile_lines("single_window")
    print("packed", packed, "contiguous", contig)
    assert packed[0] < contig[0]
    assert packed[1][0] == 0 and contig[1][0] == 0      # no tile in global-atomics mode


@pytest.mark.parametrize("case,env", [("two_windows", None), ("single_window", {"SADVIO_TILE_ROUNDS": "4"}), ("sharded", None)])
def test_other_regimes_keep_the_contiguous_cut(case, env):
    packed, contig = _tile_lines(case, env)
    assert packed == contig
