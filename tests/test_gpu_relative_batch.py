"""sadvio_ba_marginalize_relative_batch on the GPU: every pair factor of a window in one call, against the oracle's single-pair
routine (oracle.marginalize_relative, pinned on the reference's formulas by tests/test_oracle_relative.py).

Bars (those of tests/test_gpu_relative.py): max|Ak - Ak_ref| <= 1e-9 max|Ak_ref|, max|inf - inf_ref| <= 1e-7 max|inf_ref|.
inf is compared in the noise-floor mode only, and only for pairs whose oracle inf has numpy.linalg.cond <= 1e7: above that (and
always in the reference mode, cond 1e14 .. 1e17) inf is rounding noise in the oracle too. For those pairs Ak, n_shared and T_a_b
are still compared, and status need only be OK or REFUSED (a refused pair then has zeros, as the header says).
Every test prints its worst figure before asserting."""
import ctypes as C

import numpy as np
import pytest

from sadvio_amd import capi, synthetic

pytestmark = pytest.mark.gpu
AK_TOL, INF_TOL, COND_MAX = 1e-9, 1e-7, 1e7
OK, REFUSED = capi.SADVIO_OK, capi.E_REFUSED
_ip = C.POINTER(C.c_int32)
_dp = C.POINTER(C.c_double)


def shared_counts(w, a, b):
    """(distinct landmarks both key-frames observe, how many of them have more than one feature in b) from the window arrays."""
    n_shared = n_multi = 0
    for l in range(w.n_lmk):
        kf = w.obs_kf[w.lmk_obs_ptr[l]:w.lmk_obs_ptr[l + 1]]
        ca, cb = int((kf == a).sum()), int((kf == b).sum())
        if ca and cb:
            n_shared += 1
            n_multi += cb > 1
    return n_shared, n_multi


def T_a_b_of(w, a, b):
    return synthetic.T_to_12(synthetic.T12_to_4(w.kf_T_f_w[a]) @ synthetic.inv4(synthetic.T12_to_4(w.kf_T_f_w[b])))


def is_zero(got, i):
    return not (got["inf"][i].any() or got["Ak"][i].any() or got["T_a_b"][i].any() or got["n_shared"][i])


def check_pair(got, i, w, a, b, ref, compare_inf, fig):
    """Pair i of a batch result against the oracle's (inf, Ak, m) or None. Returns True when inf was compared. fig collects the
    worst relative differences."""
    st = int(got["status"][i])
    if ref is None:
        assert st == REFUSED and is_zero(got, i), f"pair ({a}, {b}): the oracle refuses, got status {st}"
        return False
    cond = np.linalg.cond(ref[0])
    well = compare_inf and cond <= COND_MAX
    if well:
        assert st == OK, f"pair ({a}, {b}): status {st}, oracle cond {cond:.2e}"
    else:
        assert st in (OK, REFUSED)
        if st == REFUSED:
            assert is_zero(got, i)
            return False
    e_ak = np.abs(got["Ak"][i] - ref[1]).max() / np.abs(ref[1]).max()
    fig["Ak"] = max(fig.get("Ak", 0.0), e_ak)
    fig["T"] = max(fig.get("T", 0.0), np.abs(got["T_a_b"][i] - T_a_b_of(w, a, b)).max())
    assert e_ak <= AK_TOL, f"pair ({a}, {b}): |Ak - ref| / max = {e_ak:.3e}"
    assert np.abs(got["T_a_b"][i] - T_a_b_of(w, a, b)).max() <= 1e-14
    if well:
        e_inf = np.abs(got["inf"][i] - ref[0]).max() / np.abs(ref[0]).max()
        fig["inf"] = max(fig.get("inf", 0.0), e_inf)
        fig["cond"] = max(fig.get("cond", 0.0), cond)
        assert e_inf <= INF_TOL, f"pair ({a}, {b}): |inf - ref| / max = {e_inf:.3e} at cond {cond:.2e}"
    return well


@pytest.mark.parametrize("factor", [capi.FACTOR_PIXEL, capi.FACTOR_ANGULAR])
def test_parity_all_ordered_pairs(backend_cls, oracle_lib, factor):
    w = synthetic.make_window(n_kf=5, n_lmk=300, obs_per_lmk=6, seed=14, factor=factor)
    pairs = [(a, b) for a in range(5) for b in range(5) if a != b]
    be = backend_cls(device=0)
    try:
        be.set_windows([w])
        got = be.marginalize_relative_batch(0, pairs)
        got_ref_mode = be.marginalize_relative_batch(0, pairs, eig_cut="reference")
    finally:
        be.close()
    fig, n_inf, n_live, n_multi_pairs = {}, 0, 0, 0
    for i, (a, b) in enumerate(pairs):
        ref = oracle_lib.marginalize_relative(w, a, b)
        n_sh, n_multi = shared_counts(w, a, b)
        n_multi_pairs += n_multi > 0
        assert (ref is None) == (n_sh == 0)
        if ref is not None:
            n_live += 1
            if got["status"][i] == OK:
                assert got["n_shared"][i] == n_sh
        n_inf += check_pair(got, i, w, a, b, ref, True, fig)
        ref0 = oracle_lib.marginalize_relative(w, a, b, eig_cut="reference")
        assert (ref0 is None) == (ref is None)
        check_pair(got_ref_mode, i, w, a, b, ref0, False, fig)
        if ref0 is not None and got_ref_mode["status"][i] == OK:
            assert got_ref_mode["n_shared"][i] == n_sh
    print(f"factor {factor}: {n_live} live pairs, inf compared on {n_inf}, worst {fig}")
    for a, b in ((0, 4), (4, 0)):
        assert got["status"][pairs.index((a, b))] == REFUSED
    assert n_live == 18 and n_live - n_inf <= 2
    assert n_multi_pairs >= 1


STRIDE_N = [1, 2, 3, 4, 15, 16, 17, 63, 64, 65, 255, 256, 257, 1023, 1024, 1025]   # 16 lane groups, 64 rows per pass, 256 threads


@pytest.mark.parametrize("n", STRIDE_N)
def test_item_counts_at_the_kernel_strides(backend_cls, oracle_lib, n):
    w = synthetic.make_window(n_kf=2, n_lmk=n, obs_per_lmk=4, seed=31)
    pairs = [(0, 1), (1, 0)]
    be = backend_cls(device=0)
    try:
        be.set_windows([w])
        got = be.marginalize_relative_batch(0, pairs)
    finally:
        be.close()
    fig, n_inf = {}, 0
    for i, (a, b) in enumerate(pairs):
        assert shared_counts(w, a, b) == (n, n)              # every landmark: both cameras of both key-frames
        ref = oracle_lib.marginalize_relative(w, a, b)
        assert ref is not None and ref[2] == 6 * n           # m = 3 * sum of multiplicities
        n_inf += check_pair(got, i, w, a, b, ref, True, fig)
        if got["status"][i] == OK:
            assert got["n_shared"][i] == n
    print(f"N = {n}: inf compared on {n_inf} of 2, worst {fig}")
    if n >= 4 and n not in (15, 16, 17):                     # oracle cond <= 3.8e6 measured for these
        assert n_inf == 2


def test_refusal_inside_a_batch_and_independence(backend_cls, oracle_lib):
    w = synthetic.make_window(n_kf=12, n_lmk=60, obs_per_lmk=3, seed=2, band=1, length=40.0)
    pairs = [(0, 1), (0, 11), (5, 6), (3, 5), (10, 11), (1, 0)]
    live = [p for p in pairs if p not in ((0, 11), (3, 5))]
    be = backend_cls(device=0)
    try:
        be.set_windows([w])
        got = be.marginalize_relative_batch(0, pairs)
        alone = be.marginalize_relative_batch(0, live)
    finally:
        be.close()
    fig = {}
    for i, (a, b) in enumerate(pairs):
        ref = oracle_lib.marginalize_relative(w, a, b)
        assert (ref is None) == ((a, b) in ((0, 11), (3, 5)))
        check_pair(got, i, w, a, b, ref, True, fig)
        if ref is not None:
            assert got["status"][i] == OK
    print(f"worst {fig}")
    for j, p in enumerate(live):
        i = pairs.index(p)
        for key in ("inf", "Ak", "T_a_b", "n_shared", "status"):
            assert np.array_equal(got[key][i], alone[key][j]), f"pair {p}: {key} depends on the rest of the batch"


def test_determinism_and_a_grid_beyond_the_cu_count(backend_cls, oracle_lib):
    w = synthetic.make_window(n_kf=40, n_lmk=3000, length=20.0, band=6, seed=5, pixel_noise=0.5)
    base = [(k, k + s) for k in range(w.n_kf - 1) for s in (1, 2) if k + s < w.n_kf]
    assert len(base) == 77
    pairs = [base[i % 77] for i in range(1001)]
    keys = ("inf", "Ak", "T_a_b", "n_shared", "status")
    be = backend_cls(device=0)
    try:
        be.set_windows([w])
        got = be.marginalize_relative_batch(0, pairs)
        again = be.marginalize_relative_batch(0, pairs)
        rev = be.marginalize_relative_batch(0, pairs[::-1])
        spots = list(range(0, 77, 13))
        single = [be.marginalize_relative(0, *base[i]) for i in spots]
    finally:
        be.close()
    assert (got["status"] == OK).all()
    for key in keys:
        assert np.array_equal(got[key], again[key]), f"{key}: a second call differs"
        assert np.array_equal(got[key], rev[key][::-1]), f"{key}: the reversed pair list differs"
        for i in range(77, 1001):
            assert np.array_equal(got[key][i], got[key][i % 77]), f"{key}: duplicate {i} differs from its first occurrence"
    fig, fig1 = {}, {}
    for i, one in zip(spots, single):
        a, b = base[i]
        ref = oracle_lib.marginalize_relative(w, a, b)
        assert ref is not None and one is not None
        assert got["n_shared"][i] == shared_counts(w, a, b)[0]
        check_pair(got, i, w, a, b, ref, True, fig)
        e_ak = np.abs(one[1] - ref[1]).max() / np.abs(ref[1]).max()
        fig1["Ak"] = max(fig1.get("Ak", 0.0), e_ak)
        assert e_ak <= AK_TOL
        if np.linalg.cond(ref[0]) <= COND_MAX:
            e_inf = np.abs(one[0] - ref[0]).max() / np.abs(ref[0]).max()
            fig1["inf"] = max(fig1.get("inf", 0.0), e_inf)
            assert e_inf <= INF_TOL
    print(f"batch worst {fig}; single-pair call worst {fig1}; shared landmarks {got['n_shared'][:77].min()} .. {got['n_shared'][:77].max()}")


def test_the_solve_state_is_left_alone(backend_cls):
    w = synthetic.make_window(n_kf=5, n_lmk=300, obs_per_lmk=6, seed=14)
    pairs = [(a, b) for a in range(5) for b in range(5) if a != b]
    opts = capi.reference_options()
    be = backend_cls(device=0)
    try:
        be.set_windows([w])
        be.solve(opts)
        d0 = be.get_deltas(0)
        be.marginalize_relative_batch(0, pairs)
        d1 = be.get_deltas(0)
    finally:
        be.close()
    for key in d0:
        assert np.array_equal(d0[key], d1[key]), key
    be = backend_cls(device=0, use_graph=True)
    try:
        be.set_windows([w])
        s0 = be.solve(opts)[0]
        be.marginalize_relative_batch(0, pairs)
        s1 = be.solve(opts)[0]
    finally:
        be.close()
    # The same summary: the counts exactly; the costs to 1e-9 relative, the bar this suite holds a repeated solve to (test_gpu_edges.py:
    # the tiles' atomics into S land in a different order every run, so two solves of one handle differ in the last bits of the cost
    # with or without a call between them; measured here: 9e-16).
    ints = ("iterations", "num_successful_steps", "num_unsuccessful_steps", "termination")
    worst = max(abs(getattr(s0, f) - getattr(s1, f)) / max(abs(getattr(s0, f)), 1e-300) for f in ("initial_cost", "final_cost", "fixed_cost", "final_radius"))
    print(f"second solve after the batch call: counts {[getattr(s1, f) for f in ints]}, worst relative cost difference {worst:.2e}")
    assert [getattr(s0, f) for f in ints] == [getattr(s1, f) for f in ints]
    assert worst <= 1e-9


def raw_call(be, w, ka, kb, mode=1, null_inf=False, null_status=False):
    n = len(ka)
    ka = np.ascontiguousarray(ka, dtype=np.int32); kb = np.ascontiguousarray(kb, dtype=np.int32)
    out = {"inf": np.full((max(n, 1), 36), 7.0), "Ak": np.full((max(n, 1), 144), 7.0), "T_a_b": np.full((max(n, 1), 12), 7.0),
           "n_shared": np.full(max(n, 1), 7, dtype=np.int32), "status": np.full(max(n, 1), 7, dtype=np.int32)}
    rc = be.lib.sadvio_ba_marginalize_relative_batch(
        be.h, w, n, ka.ctypes.data_as(_ip), kb.ctypes.data_as(_ip), mode, _dp() if null_inf else out["inf"].ctypes.data_as(_dp),
        out["Ak"].ctypes.data_as(_dp), out["T_a_b"].ctypes.data_as(_dp), out["n_shared"].ctypes.data_as(_ip),
        _ip() if null_status else out["status"].ctypes.data_as(_ip))
    untouched = all((v == 7).all() for v in out.values())
    return rc, untouched


def test_arguments(backend_cls):
    from vio_helpers import make_vio_window
    w = synthetic.make_window(n_kf=5, n_lmk=300, obs_per_lmk=6, seed=14)
    be = backend_cls(device=0)
    try:
        assert raw_call(be, 0, [0], [1]) == (capi.E_STATE, True)                      # before set_windows
        be.set_windows([w])
        assert raw_call(be, 0, [], []) == (OK, True)                                  # n_pair = 0
        assert raw_call(be, 0, [0], [1])[0] == OK
        for ka, kb in (([0, 2], [1, 2]), ([0, -1], [1, 2]), ([0, 1], [1, -1]), ([0, 5], [1, 2]), ([0, 1], [1, 5])):
            assert raw_call(be, 0, ka, kb) == (capi.E_INVALID_ARG, True), (ka, kb)
        assert raw_call(be, 0, [0], [1], mode=2) == (capi.E_INVALID_ARG, True)
        assert raw_call(be, 0, [0], [1], null_inf=True) == (capi.E_INVALID_ARG, True)
        assert raw_call(be, 0, [0], [1], null_status=True) == (capi.E_INVALID_ARG, True)
        assert raw_call(be, 1, [0], [1]) == (capi.E_INVALID_ARG, True)                # window out of range
        be._check(be.lib.sadvio_ba_begin_update(be.h), "begin_update")
        r = raw_call(be, 0, [0], [1])
        be._check(be.lib.sadvio_ba_commit_update(be.h), "commit_update")
        assert r == (capi.E_STATE, True)
        assert raw_call(be, 0, [0], [1])[0] == OK
    finally:
        be.close()
    wi = make_vio_window(n_kf=4, n_lmk=60)
    be = backend_cls(device=0)
    try:
        be.set_windows([wi])
        assert raw_call(be, 0, [0], [1]) == (capi.E_INVALID_ARG, True)                # has_imu
    finally:
        be.close()
