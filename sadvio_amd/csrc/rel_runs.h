// rel_runs.h — where two key-frames sit in a long track's observation range. layout_sort (layout_plan.h) leaves every landmark's device
// range sorted ascending by key-frame, and a long track carries real observations only, so the observations of key-frames ga and gb
// are two runs that bisection on obs_kf finds in O(log n) reads instead of a walk over up to 4 096 observations. Used by the relative
// marginalisations (rel_kernels.h: rel_linearise; marg_kernels.h: k_relmarg_lmk; marg_driver.h: marginalize_relative) for landmarks of
// more than MAX_LMK_OBS observations; the runs come back in ascending position, so a caller that visits run 0 and then run 1 visits
// exactly the observations the walk would stop at, in the walk's order, and every sum it forms has the walk's bits.
// Compiles without HIP (tests/cpp/test_rel_runs.cpp).
#pragma once

#if defined(__HIPCC__)
#define SADVIO_REL_HD __host__ __device__
#else
#define SADVIO_REL_HD
#endif

namespace sadvio {

struct RelRuns {
    int lo[2], hi[2];   // run r is [lo[r], hi[r]); run 0 lies in front of run 1; an absent key-frame has an empty run
};

// first position in [lo, hi) whose key-frame is at least kf (hi: none); obs_kf ascending on [lo, hi)
SADVIO_REL_HD inline int rel_first_at_least(const int* obs_kf, int lo, int hi, int kf) {
    while (lo < hi) {
        const int mid = lo + (hi - lo) / 2;
        if (obs_kf[mid] < kf) lo = mid + 1; else hi = mid;
    }
    return lo;
}

// one past the last observation of key-frame kf's run, which begins at lo
SADVIO_REL_HD inline int rel_run_end(const int* obs_kf, int lo, int oe, int kf) {
    const int hi = rel_first_at_least(obs_kf, lo, oe, kf + 1);
#ifdef PLANT_SHORT_RUN   // (tests/cpp/test_rel_runs.cpp alone defines it: an off-by-one that its comparison has to see)
    return hi > lo ? hi - 1 : hi;
#else
    return hi;
#endif
}

// The runs of key-frames ga and gb (ga != gb, either order) inside [ob, oe)
SADVIO_REL_HD inline RelRuns rel_runs(const int* obs_kf, int ob, int oe, int ga, int gb) {
    const int k0 = ga < gb ? ga : gb, k1 = ga < gb ? gb : ga;
    RelRuns R;
    R.lo[0] = rel_first_at_least(obs_kf, ob, oe, k0);
    R.hi[0] = rel_run_end(obs_kf, R.lo[0], oe, k0);
    R.lo[1] = rel_first_at_least(obs_kf, R.hi[0], oe, k1);
    R.hi[1] = rel_run_end(obs_kf, R.lo[1], oe, k1);
    return R;
}

}  // namespace sadvio
