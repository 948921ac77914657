"""The host-only planner (sadvio_amd/csrc/layout_plan.h) with long tracks, through tests/cpp/dump_long_plan.cpp (plain g++, no GPU):
  - exactly the landmarks with at least SADVIO_LONG_MIN observations are on the long list, every other landmark is in exactly one tile,
    and the long list's key-frame lists and observation slots are those of the key-frame-sorted observations;
  - the tiles of MIX are the tiles of MIX with its long tracks emptied (no observations), those landmarks apart;
  - a long track given in shuffled order is sorted without the 8-bit position field of the short tracks' sort key wrapping;
  - the documented caps have their own error texts, and a sharded layout keeps the refusal it had;
  - windows without long tracks yield, line by line, the dump that tests/cpp/dump_tile_plan.cpp printed before long tracks existed
    (tests/golden/plan_dump_before_long_tracks.txt, written from the commit before them)."""
import os
import subprocess

import numpy as np
import pytest

import long_track_helpers as lh
import step_helpers as sh
from sadvio_amd import synthetic

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN_DUMP = os.path.join(ROOT, "tests", "golden", "plan_dump_before_long_tracks.txt")


def _compile(tmp, name):
    exe = str(tmp / name)
    r = subprocess.run(["g++", "-std=c++17", "-O1", "-Wall", "-Werror", os.path.join(ROOT, "tests", "cpp", name + ".cpp"), "-o", exe], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    return exe


@pytest.fixture(scope="module")
def dump_long_plan(tmp_path_factory):
    exe = _compile(tmp_path_factory.mktemp("long_plan"), "dump_long_plan")

    def run(ws, long_min=65, env=None):
        p = subprocess.run([exe], input=f"{long_min}\n" + sh.plan_input(ws, env or {}), capture_output=True, text=True)
        assert p.returncode == 0, p.stderr
        return parse(p.stdout)
    return run


def parse(text):
    ints = lambda s: [int(v) for v in s.split()]
    plan = {"tiles": [], "long": [], "obs": {}, "error": None}
    for line in text.splitlines():
        if line.startswith("E "):
            plan["error"] = line[2:]
            continue
        parts = line[2:].split("|")
        h = ints(parts[0])
        if line[0] == "P":
            plan.update(zip(("n_tiles", "n_long", "long_max_kf", "lm_ok"), h))
        elif line[0] == "L":
            plan["long"].append(dict(zip(("w", "lmk", "n_obs", "n_kf"), h[1:]), kfs=ints(parts[1]), slots=ints(parts[2])))
        elif line[0] == "T":
            plan["tiles"].append(dict(zip(("w", "lds_mode", "G", "n_lmk", "n_free", "n_kf", "kmax", "listed"), h[1:]), kfs=ints(parts[1]), rows=ints(parts[2]),
                                      lmks=ints(parts[3])))
        elif line[0] == "O":
            plan["obs"][h[0]] = (ints(parts[1]), ints(parts[2]))
    return plan


def emptied(w, which):
    """w with the landmarks `which` left without observations (same indices)."""
    import test_gpu_tile_packing as tp
    none = np.arange(0)
    e = tp._assemble(w, [(w, l, none if l in set(which) else None) for l in range(w.n_lmk)])
    e.lmk_const = getattr(w, "lmk_const", None)
    return e


@pytest.mark.parametrize("long_min", [65, 6, 5])
def test_long_list_holds_exactly_the_landmarks_at_or_above_the_threshold(dump_long_plan, long_min):
    w = lh.case_window(lh.CASE["MIX"])
    plan = dump_long_plan([w], long_min)
    n = lh.counts(w)
    want = np.flatnonzero(n >= long_min).tolist()
    assert [t["lmk"] for t in plan["long"]] == want and plan["n_long"] == len(want)
    in_tiles = sorted(l for t in plan["tiles"] for l in t["lmks"])
    assert in_tiles == [l for l in range(w.n_lmk) if l not in want]          # every other landmark in exactly one tile
    assert all(t["n_lmk"] == len(t["lmks"]) and t["listed"] == (1 if want else t["listed"]) for t in plan["tiles"])
    assert all(t["kmax"] <= 64 and t["n_kf"] <= 24 for t in plan["tiles"])
    assert plan["lm_ok"] == 0
    obs_kf, perm = plan["obs"][0]
    assert sorted(perm) == list(range(len(w.obs_kf)))
    for t in plan["long"]:
        l = t["lmk"]
        o = np.arange(w.lmk_obs_ptr[l], w.lmk_obs_ptr[l + 1])
        order = o[np.argsort(w.obs_kf[o], kind="stable")]                      # the stable key-frame sort of the landmark's list
        assert perm[o[0]:o[-1] + 1] == order.tolist()
        assert obs_kf[o[0]:o[-1] + 1] == w.obs_kf[order].tolist()
        kfs = sorted(set(w.obs_kf[o].tolist()))
        assert t["kfs"] == kfs and t["n_kf"] == len(kfs) and t["n_obs"] == len(o)
        assert [kfs[s] for s in t["slots"]] == w.obs_kf[order].tolist()
    assert plan["long_max_kf"] == max([t["n_kf"] for t in plan["long"]], default=0)


def test_tiles_of_mix_are_the_tiles_of_mix_with_its_long_tracks_emptied(dump_long_plan):
    w = lh.case_window(lh.CASE["MIX"])
    long_ = lh.long_landmarks(w).tolist()
    a = dump_long_plan([w])
    b = dump_long_plan([emptied(w, long_)])
    assert b["n_long"] == 0 and a["n_long"] == 3 and len(a["tiles"]) == len(b["tiles"])
    key = ("w", "lds_mode", "G", "n_free", "n_kf", "kmax", "listed", "kfs", "rows")
    for ta, tb in zip(a["tiles"], b["tiles"]):
        assert [ta[k] for k in key] == [tb[k] for k in key]
        assert ta["lmks"] == [l for l in tb["lmks"] if l not in long_]
    # and in a batch (the contiguous cut), where window 1 holds the long tracks
    w0 = synthetic.make_window(n_kf=5, n_lmk=40, seed=3)
    a = dump_long_plan([w0, w])
    b = dump_long_plan([w0, emptied(w, long_)])
    assert [t["lmk"] for t in a["long"]] == long_ and all(t["w"] == 1 for t in a["long"]) and len(a["tiles"]) == len(b["tiles"])
    for ta, tb in zip(a["tiles"], b["tiles"]):
        assert [ta[k] for k in key if k != "listed"] == [tb[k] for k in key if k != "listed"]
        assert ta["lmks"] == [l for l in tb["lmks"] if not (tb["w"] == 1 and l in long_)]
        assert ta["listed"] == (1 if ta["w"] == 1 else 0)


def test_a_window_of_long_tracks_only_keeps_one_empty_tile(dump_long_plan):
    plan = dump_long_plan([lh.case_window(lh.CASE["L65"])])
    assert plan["n_long"] == 12 and [t["n_lmk"] for t in plan["tiles"]] == [0] and plan["tiles"][0]["n_kf"] == 0


def _shuffled_long_window(n_obs, n_kf=200, seed=5):
    """One landmark of n_obs observations in shuffled order (and a short one), every key-frame constant but two: structure only."""
    rng = np.random.default_rng(seed)
    w = synthetic.make_window(n_kf=4, n_lmk=2, obs_per_lmk=4, seed=1)
    views = rng.permutation(2 * n_kf)[:n_obs] if n_obs <= 2 * n_kf else rng.integers(0, 2 * n_kf, n_obs)   # (repeated views: the planner does not mind)
    kc = np.ones(n_kf, dtype=np.uint8); kc[:2] = 0
    w.kf_const = kc
    w.kf_T_f_w = np.tile(w.kf_T_f_w[0], (n_kf, 1))
    w.obs_kf = np.concatenate([views // 2, [0, 0, 1, 1]]).astype(np.int32)
    w.obs_cam = np.concatenate([views % 2, [0, 1, 0, 1]]).astype(np.int32)
    w.obs_meas = np.zeros((n_obs + 4, 2))
    w.lmk_obs_ptr = np.array([0, n_obs, n_obs + 4], dtype=np.int32)
    return w


def test_a_shuffled_long_track_is_sorted_past_256_observations(dump_long_plan):
    w = _shuffled_long_window(300)
    plan = dump_long_plan([w])
    assert plan["error"] is None and [t["lmk"] for t in plan["long"]] == [0]
    obs_kf, perm = plan["obs"][0]
    order = np.argsort(w.obs_kf[:300], kind="stable")
    assert perm[:300] == order.tolist() and obs_kf[:300] == w.obs_kf[order].tolist()
    assert len(set(perm[:300])) == 300


def test_caps_and_the_sharded_refusal_have_their_own_texts(dump_long_plan):
    e = dump_long_plan([lh.case_window(lh.CASE["L65"])], long_min=0)["error"]      # the planner's default: no long path, the refusal it always gave
    assert e == "set_windows: a landmark has more than 64 observations"
    e = dump_long_plan([_shuffled_long_window(lh.MAX_LONG_OBS + 1)])["error"]
    assert e is not None and "long track" in e and str(lh.MAX_LONG_OBS) in e and "observations" in e
    p = dump_long_plan([_shuffled_long_window(lh.MAX_LONG_OBS)])
    assert p["error"] is None and p["long"][0]["n_obs"] == lh.MAX_LONG_OBS
    at_kf = _shuffled_long_window(2 * lh.MAX_LONG_KF, n_kf=lh.MAX_LONG_KF)
    p = dump_long_plan([at_kf])
    assert p["error"] is None and p["long_max_kf"] == lh.MAX_LONG_KF
    over_kf = _shuffled_long_window(2 * lh.MAX_LONG_KF + 2, n_kf=lh.MAX_LONG_KF + 1)
    e = dump_long_plan([over_kf])["error"]
    assert e is not None and "long track" in e and str(lh.MAX_LONG_KF) in e and "key-frames" in e


def test_windows_without_long_tracks_get_the_plan_they_had(tmp_path):
    """dump_tile_plan's output on windows without long tracks, against what the same program printed on the commit before long tracks
    (single packed windows, the contiguous cut of a batch, multi-round tiles, the throughput tables, 64-observation landmarks)."""
    exe = _compile(tmp_path, "dump_tile_plan")
    got = []
    for name, ws, env in plan_dump_inputs():
        p = subprocess.run([exe], input=sh.plan_input(ws, env), capture_output=True, text=True)
        assert p.returncode == 0, p.stderr
        got.append(f"# {name}\n{p.stdout}")
    with open(GOLDEN_DUMP) as f:
        assert "".join(got) == f.read()


def plan_dump_inputs():
    import test_gpu_tile_packing as tp
    w70 = sh.case_window(sh.CASE["w70"])
    g64 = sh.case_window(sh.CASE["g64"])
    out = [("w70", [w70], {}), ("w70 contiguous", [w70], {"SADVIO_CONTIG_TILES": "1"}), ("w70 throughput", [w70], {"SADVIO_LM": "1"}),
           ("w70 three rounds", [w70], {"SADVIO_TILE_ROUNDS": "3"}), ("g64", [g64], {}), ("outliers", [tp.make_case("outliers")], {}),
           ("batch", [tp.make_case("g16"), w70, tp.make_case("disjoint")], {}),
           ("mix without its long tracks", [lh.mix_short()], {})]
    return out
