"""The host-only planner of the covariance's border route (sadvio_amd/csrc/cov_border_plan.h) through
tests/cpp/dump_cov_border_plan.cpp (plain g++, no GPU; once more under the address and undefined-behaviour sanitizers), against hand-made
cases and against the rule restated in cov_border_helpers.plan_rule on the windows of the GPU tests and on seeded random couplings."""
import os
import subprocess

import numpy as np
import pytest

import cov_band_helpers as cb
import cov_border_helpers as bh

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module", params=[False, True], ids=["plain", "sanitized"])
def dump(request, tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("cov_border_plan") / "dump_cov_border_plan")
    flags = ["-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-g"] if request.param else []
    r = subprocess.run(["g++", "-std=c++17", "-O1", "-Wall", "-Werror", *flags, os.path.join(ROOT, "tests", "cpp", "dump_cov_border_plan.cpp"), "-o", exe],
                       capture_output=True, text=True)
    assert r.returncode == 0, r.stderr

    def run(n_free, cliques, pairs, dpf=6, nb=6, hb_lim=19, fills=False):
        p = subprocess.run([exe], input=bh.plan_input(n_free, cliques, pairs, dpf, nb, hb_lim, fills), capture_output=True, text=True)
        assert p.returncode == 0, p.stdout + p.stderr
        return bh.parse_plan(p.stdout)
    return run


def chain(n, reach=1):
    """Landmark cliques of a chain of n free key-frames: every run of reach + 1 consecutive key-frames shares a landmark."""
    return [list(range(k, k + reach + 1)) for k in range(n - reach)]


def test_chain_with_one_closure_factor(dump):
    p = dump(40, chain(40, 2), [(3, 33)], hb_lim=5)
    assert p.answer == "OK" and p.border == [3] and p.n_edges == 1 and p.hb_core == 2
    assert p.core_of[:5] == [0, 1, 2, -1, 3] and p.order[-1] == 3 and p.order[:4] == [0, 1, 2, 4] and p.n_core == 39


def test_landmark_seen_from_both_ends_takes_three_not_six(dump):
    p = dump(40, chain(40, 2) + [[3, 4, 5, 30, 31, 32]], [], hb_lim=5)
    assert p.answer == "OK" and p.n_edges == 9 and p.border == [3, 4, 5]          # all six tie at three edges: the lowest indices
    # ... and with a second landmark that makes the far side the better cover, the far side is taken
    p = dump(40, chain(40, 2) + [[3, 4, 5, 30, 31, 32], [10, 30, 31, 32]], [], hb_lim=5)
    assert p.border == [30, 31, 32] and p.n_edges == 12


def test_ties_take_the_lowest_index(dump):
    p = dump(30, chain(30), [(20, 2), (25, 7)], hb_lim=4)
    assert p.border == [2, 7]
    p = dump(30, chain(30), [(2, 20), (2, 25), (9, 25)], hb_lim=4)                # 2 and 25 cover two each: 2 first, then 9 before 25
    assert p.border == [2, 9]


def test_core_band_holds_by_construction(dump):
    rng = np.random.default_rng(7)
    for _ in range(40):
        n = int(rng.integers(20, 60))
        reach = int(rng.integers(1, 4))
        hb_lim = int(rng.integers(reach, 8))
        pairs = [tuple(int(v) for v in rng.choice(n, 2, replace=False)) for _ in range(int(rng.integers(1, 4)))]
        cliques = chain(n, reach) + [sorted(int(v) for v in rng.choice(n, 4, replace=False)) for _ in range(int(rng.integers(0, 3)))]
        for k in cliques:                                                          # (repeats, any order and a constant key-frame are the planner's to clean)
            if rng.random() < 0.3:
                k += [k[0], -1]
                rng.shuffle(k)
        got = dump(n, cliques, pairs, hb_lim=hb_lim)
        clean = [sorted(set(v for v in k if v >= 0)) for k in cliques]
        want = bh.plan_rule(n, clean, [(min(a, b), max(a, b)) for a, b in pairs], 6, 6, hb_lim)
        assert got == want, (n, cliques, pairs, hb_lim)
        if got.answer == "OK":
            assert got.hb_core <= hb_lim and len(got.border) * 6 <= bh.COV_BORDER_MAXM
            b = set(got.border)
            for k in clean:
                for i, a in enumerate(k):
                    for c in k[i + 1:]:
                        assert a in b or c in b or got.core_of[c] - got.core_of[a] <= got.hb_core
            assert sorted(got.order) == list(range(n)) and got.order[got.n_core:] == got.border


def test_not_borderable_answers(dump):
    far = [(k, k + 25) for k in range(0, 34, 2)]                                   # 17 disjoint closure edges: 17 border key-frames, m = 102
    assert dump(60, chain(60), far, hb_lim=4).answer == "TOO_WIDE"
    assert dump(60, chain(60), far[:16], hb_lim=4).answer == "OK"                  # m = 96 fits
    assert dump(60, chain(60), far[:7], dpf=15, nb=5, hb_lim=4).answer == "TOO_WIDE"   # 7 x 15 = 105
    filled = dump(40, chain(40), [(3, 33)], hb_lim=5, fills=True)                  # a dense prior, kept landmarks or lines
    assert filled.answer == "FILLED" and filled.border == [] and filled.order == list(range(40))
    assert dump(40, chain(40), [(3, 33)], nb=4, hb_lim=5).answer == "CORE_SHAPE"   # n_b = 234 is no multiple of 4
    assert dump(4, chain(4, 2), [(0, 3)], hb_lim=2).answer == "CORE_SHAPE"         # core {1, 2, 3}: n_b = 18 is not above bw' = 18
    plain = dump(40, chain(40, 2), [(3, 8)], hb_lim=5)
    assert plain.answer == "PLAIN" and plain.border == [] and plain.hb_core == 5 and plain.core_of == list(range(40))


@pytest.mark.parametrize("case", list(bh.WINDOWS))
def test_windows_of_the_gpu_tests(dump, case):
    build, _, hb = bh.WINDOWS[case]
    w = build()
    dpf = 15 if w.has_imu else 6
    cliques, pairs = bh.couplings(w)
    n_free = int((cb.free_index(w) >= 0).sum())
    got = dump(n_free, cliques, pairs, dpf=dpf, nb=cb.block_column(dpf), hb_lim=hb)
    assert got == bh.plan_of(w, hb) and got.answer == "OK" and got.hb_core <= hb
    # at the band kernels' own limit a window whose hb fits has no closure edge: plainly bandable, an empty border (closure40's
    # factor spans 30 key-frames and stays a closure edge)
    plain = dump(n_free, cliques, pairs, dpf=dpf, nb=cb.block_column(dpf), hb_lim=bh.hb_max(dpf))
    if cb.bandwidth(w)[0] <= bh.hb_max(dpf):
        assert plain.answer == "PLAIN" and plain.border == [] and plain.hb_core == cb.bandwidth(w)[0]
    else:
        assert case == "closure40" and plain.answer == "OK" and plain.border == got.border


def test_at_size_closure_window(dump):
    w = bh.window_at_size_closure()
    cliques, pairs = bh.couplings(w)
    got = dump(344, cliques, pairs)
    a, _ = bh.AT_SIZE_CLOSURE_KF
    assert got == bh.plan_of(w) and got.answer == "OK" and got.border == [a] and got.n_core * 6 == 2058 and got.hb_core <= 19
