// Stand-alone check of sadvio_amd/csrc/cov_cross_plan.h (host only): the launch tables of sadvio_ba_covariance_cross against a
// brute-force restatement, on hand-made and seeded random requests. Prints OK.
#include <algorithm>
#include <cstdio>
#include <map>
#include <random>
#include <vector>

#include "../../sadvio_amd/csrc/cov_cross_plan.h"

static int fails = 0;
#define CHECK(c) do { if (!(c)) { std::printf("FAILED %s:%d %s\n", __FILE__, __LINE__, #c); fails++; } } while (0)

static void check_case(const std::vector<int>& kf, const std::vector<int>& fidx, int per_wg) {
    const int n = (int)kf.size(), n_kf = (int)fidx.size();
    sadvio::CovCrossPlan P;
    P.order = {97, 98}; P.groups = {1}; P.wgs = {2, 3}; P.rows = {5};   // stale contents must not survive
    sadvio::cov_cross_plan(n, kf.data(), n_kf, fidx.data(), per_wg, P);
    CHECK((int)P.order.size() == n);
    CHECK(P.groups.size() % 4 == 0 && P.wgs.size() % 4 == 0);
    // order is a permutation of the request positions
    std::vector<int> seen((size_t)n, 0);
    for (int c : P.order) { CHECK(c >= 0 && c < n); if (c >= 0 && c < n) seen[c]++; }
    for (int c = 0; c < n; c++) CHECK(seen[c] == 1);
    // groups: ascending key-frame, contiguous, cover [0, n), every member is the group's key-frame, request order inside
    std::map<int, std::vector<int>> want;
    for (int c = 0; c < n; c++) want[kf[c]].push_back(c);
    CHECK(P.n_group() == (int)want.size());
    int at = 0, g = 0, n_free = 0;
    for (const auto& kv : want) {
        if (g >= P.n_group()) break;
        const int* G = &P.groups[4 * (size_t)g++];
        CHECK(G[0] == kv.first && G[1] == fidx[kv.first] && G[2] == at && G[3] == at + (int)kv.second.size());
        for (size_t i = 0; i < kv.second.size() && at + (int)i < n; i++) CHECK(P.order[(size_t)at + i] == kv.second[i]);
        at += (int)kv.second.size();
        if (fidx[kv.first] >= 0) {
            CHECK(n_free < (int)P.rows.size() && P.rows[n_free] == fidx[kv.first]);
            n_free++;
        }
    }
    CHECK(at == n);
    CHECK((int)P.rows.size() == n_free);
    // workgroups: contiguous, cover [0, n), at most per_wg candidates, never across a group, the group's free index and row slot
    const int cap = std::max(per_wg, 1);
    int pos = 0;
    for (int q = 0; q < P.n_wg(); q++) {
        const int* Wg = &P.wgs[4 * (size_t)q];
        CHECK(Wg[1] == pos && Wg[2] > Wg[1] && Wg[2] - Wg[1] <= cap && Wg[2] <= n);
        if (!(Wg[1] == pos && Wg[2] > Wg[1] && Wg[2] <= n)) break;
        for (int p = Wg[1]; p < Wg[2]; p++) CHECK(fidx[kf[P.order[p]]] == Wg[0] && kf[P.order[p]] == kf[P.order[Wg[1]]]);
        if (Wg[0] < 0) CHECK(Wg[3] == -1);
        else CHECK(Wg[3] >= 0 && Wg[3] < (int)P.rows.size() && P.rows[Wg[3]] == Wg[0]);
        pos = Wg[2];
    }
    CHECK(pos == n);
    // the fewest workgroups that rule allows
    int fewest = 0;
    for (const auto& kv : want) fewest += ((int)kv.second.size() + cap - 1) / cap;
    CHECK(P.n_wg() == fewest);
}

int main() {
    // key-frame 0 constant; unsorted candidates with repeats; key-frame 2 a group of one
    check_case({3, 1, 3, 2, 1, 3, 1}, {-1, 0, 1, 2}, 96);
    // a constant key-frame among the candidates
    check_case({0, 2, 0, 1}, {-1, 0, 1}, 96);
    // only the constant key-frame
    check_case({0, 0, 0}, {-1, 0}, 2);
    // n = 0
    check_case({}, {-1, 0, 1}, 96);
    {
        sadvio::CovCrossPlan P;
        sadvio::cov_cross_plan(0, nullptr, 0, nullptr, 96, P);
        CHECK(P.order.empty() && P.groups.empty() && P.wgs.empty() && P.rows.empty());
    }
    // one group split over several workgroups, the last one short; per_wg = 1; a per_wg below 1 counts as 1
    check_case(std::vector<int>(205, 4), {0, 1, 2, 3, 4}, 96);
    check_case({1, 1, 1, 0}, {0, 1}, 1);
    check_case({1, 1, 1, 0}, {0, 1}, 0);
    // exactly full workgroups
    check_case(std::vector<int>(64, 0), {0}, 32);
    std::mt19937 rng(11);
    for (int t = 0; t < 300; t++) {
        const int n_kf = 1 + (int)(rng() % 12), n = (int)(rng() % 300), per_wg = 1 + (int)(rng() % 40);
        std::vector<int> fidx((size_t)n_kf, -1), kf((size_t)n);
        int nf = 0;
        for (int k = 0; k < n_kf; k++) if (rng() % 4) fidx[k] = nf++;
        for (int c = 0; c < n; c++) kf[c] = (int)(rng() % n_kf);
        check_case(kf, fidx, per_wg);
    }
    if (fails) return 1;
    std::printf("OK\n");
    return 0;
}
