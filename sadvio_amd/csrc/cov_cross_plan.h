// cov_cross_plan.h — the launch tables of sadvio_ba_covariance_cross (cov_cross_driver.h builds them per call; cov_cross_kernels.h:
// k_cov_cross reads them). Host only, no HIP: tests/cpp/test_cov_cross_plan.cpp compiles it on its own.
#pragma once
#include <algorithm>
#include <vector>

namespace sadvio {

// A pure function of the request and the window's free-index table. The candidates (key-frame kf[c], landmark lmk[c]) are grouped
// by key-frame, groups in ascending key-frame index, a group's candidates in request order; a group is cut into workgroups of at
// most per_wg candidates, so that every workgroup stages ONE block row Sigma(a, :) and serves candidates of that key-frame only.
struct CovCrossPlan {
    std::vector<int> order;    // [n] request positions, group after group: the candidate a lane serves is order[position]
    std::vector<int> groups;   // [n_group][4] key-frame | its free index (-1: constant) | first position | one past the last
    std::vector<int> wgs;      // [n_wg][4] free index of the key-frame (-1: constant) | first position | one past the last | row slot
    std::vector<int> rows;     // the distinct FREE key-frames asked for, as free indices, ascending key-frame index; a workgroup's
                               // row slot indexes this list (-1 for a constant key-frame): the band route solves one block row per entry
    int n_group() const { return (int)groups.size() / 4; }
    int n_wg() const { return (int)wgs.size() / 4; }
};

//   n, kf             the request: kf[c] in [0, n_kf) is the caller's to guarantee (cov_cross_check refuses anything else before)
//   kf_fidx           free index of the window's key-frame k at [k], -1: constant
//   per_wg            candidates per workgroup, >= 1
inline void cov_cross_plan(int n, const int* kf, int n_kf, const int* kf_fidx, int per_wg, CovCrossPlan& P) {
    P.order.clear(); P.groups.clear(); P.wgs.clear(); P.rows.clear();
    if (n <= 0 || n_kf <= 0) return;
    per_wg = std::max(per_wg, 1);
    std::vector<int> first((size_t)n_kf + 1, 0);   // counting sort by key-frame: stable, so a group keeps the request order
    for (int c = 0; c < n; c++) first[(size_t)kf[c] + 1]++;
    for (int k = 0; k < n_kf; k++) first[(size_t)k + 1] += first[k];
    P.order.assign((size_t)n, 0);
    {
        std::vector<int> at(first.begin(), first.end() - 1);
        for (int c = 0; c < n; c++) P.order[(size_t)at[kf[c]]++] = c;
    }
    for (int k = 0; k < n_kf; k++) {
        const int b = first[k], e = first[(size_t)k + 1];
        if (b == e) continue;
        const int f = kf_fidx[k];
        int slot = -1;
        if (f >= 0) { slot = (int)P.rows.size(); P.rows.push_back(f); }
        P.groups.insert(P.groups.end(), {k, f, b, e});
        for (int p = b; p < e; p += per_wg) P.wgs.insert(P.wgs.end(), {f, p, std::min(e, p + per_wg), slot});
    }
}

}  // namespace sadvio
