// Stand-alone check of sadvio_amd/csrc/cov_kf_lists.h (host only): the key-frame -> landmark lists of the square-root covariance
// assembly against a brute-force restatement, on hand-made and seeded random observation tables. Prints OK.
#include <algorithm>
#include <cstdio>
#include <cstdlib>
#include <random>
#include <set>
#include <vector>

#include "../../sadvio_amd/csrc/cov_kf_lists.h"

static int fails = 0;
#define CHECK(c) do { if (!(c)) { std::printf("FAILED %s:%d %s\n", __FILE__, __LINE__, #c); fails++; } } while (0)

// lmk_ob / lmk_oe hold absolute observation positions (the window's observations start at obs_base); obs_kf global key-frame indices
static void check_case(int n_free, int n_lmk, const std::vector<int>& ob, const std::vector<int>& oe, const std::vector<int>& obs_kf,
                       const std::vector<int>& fidx) {
    std::vector<int> ptr{99, 98}, lst{97};   // stale contents must not survive
    sadvio::cov_kf_lmk_lists(n_free, n_lmk, ob.data(), oe.data(), obs_kf.data(), fidx.data(), ptr, lst);
    CHECK((int)ptr.size() == std::max(n_free, 0) + 1);
    CHECK(ptr[0] == 0);
    std::vector<std::set<int>> want((size_t)std::max(n_free, 0));
    for (int l = 0; l < n_lmk; l++)
        for (int o = ob[l]; o < oe[l]; o++) {
            const int f = fidx[obs_kf[o]];
            if (f >= 0 && f < n_free) want[f].insert(l);
        }
    size_t total = 0;
    for (int f = 0; f < n_free; f++) {
        CHECK(ptr[f + 1] >= ptr[f]);
        const std::vector<int> got(lst.begin() + ptr[f], lst.begin() + ptr[f + 1]);
        const std::vector<int> ref(want[f].begin(), want[f].end());   // ascending, each once
        CHECK(got == ref);
        total += ref.size();
    }
    CHECK((size_t)ptr[std::max(n_free, 0)] == total);
    CHECK(lst.size() == std::max<size_t>(total, 1));
}

int main() {
    // two landmarks, stereo observations of the same key-frame (listed once), a constant key-frame (skipped), observations at a base
    check_case(2, 2, {10, 14}, {14, 16}, {0, 0, 0, 0, 0, 0, 0, 0, 0, 0, /*10*/ 5, 5, 6, 7, /*14*/ 6, 6}, {-1, -1, -1, -1, -1, 0, 1, -1});
    // nothing at all
    check_case(0, 0, {0}, {0}, {0}, {-1});
    check_case(3, 0, {0}, {0}, {0}, {0, 1, 2});
    // a landmark without observations between two others; a free index outside the window's range is skipped
    check_case(2, 3, {0, 2, 2}, {2, 2, 4}, {0, 1, 2, 0}, {0, 1, 7});
    // every landmark seen from every key-frame
    {
        std::vector<int> ob, oe, kf;
        for (int l = 0; l < 5; l++) { ob.push_back(4 * l); oe.push_back(4 * l + 4); for (int k = 0; k < 4; k++) kf.push_back(3 - k); }
        check_case(4, 5, ob, oe, kf, {0, 1, 2, 3});
    }
    std::mt19937 rng(7);
    for (int t = 0; t < 200; t++) {
        const int n_kf = 1 + (int)(rng() % 12), n_lmk = (int)(rng() % 40), base = (int)(rng() % 5), kf_base = (int)(rng() % 4);
        std::vector<int> fidx((size_t)kf_base + n_kf, -1);
        int n_free = 0;
        for (int k = 0; k < n_kf; k++) if (rng() % 4) fidx[kf_base + k] = n_free++;
        std::vector<int> ob, oe, kf((size_t)base, 0);
        for (int l = 0; l < n_lmk; l++) {
            const int m = (int)(rng() % 7);
            ob.push_back((int)kf.size());
            for (int o = 0; o < m; o++) kf.push_back(kf_base + (int)(rng() % n_kf));
            oe.push_back((int)kf.size());
        }
        if (ob.empty()) { ob.push_back(0); oe.push_back(0); }
        if (kf.empty()) kf.push_back(0);
        check_case(n_free, n_lmk, ob, oe, kf, fidx);
    }
    if (fails) return 1;
    std::printf("OK\n");
    return 0;
}
