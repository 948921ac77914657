// cov_border_plan.h — the planner of the covariance's BORDER route (cov_driver.h: cov_invert_border; cov_border_kernels.h). Host only,
// no HIP: tests/cpp/dump_cov_border_plan.cpp compiles it on its own.
//
// A long window with a loop closure has a reduced system S that is block-banded but for a few far couplings. The planner takes the
// key-frames of those couplings out of the band: with the reduced columns ordered [core | border],
//     S = [ B  C ]     B: the core key-frames in natural order, the border ones removed; block-banded with hb' <= hb_lim
//         [ C^T D ]    D: m x m dense, m = |border| * dpf
// THE RULE (deterministic; a pure function of the couplings, dpf, nb and hb_lim):
//   1. The couplings are the pairs of free key-frames that a landmark (every two of its observers), an IMU pair or a relative-pose
//      factor couples. A CLOSURE EDGE is a coupling whose two key-frames are more than hb_lim apart in natural free index.
//   2. The border is a vertex cover of the closure edges, built greedily: take the key-frame that covers the most closure edges not
//      yet covered, the lowest index on a tie; repeat until no closure edge is left uncovered.
//   3. Removing vertices never lengthens a distance: every coupling left between two core key-frames was at most hb_lim apart and is
//      at most as far apart in the compacted core index, so the core's hb' <= hb_lim holds by construction (and is recomputed here).
// BORDERABLE: nothing but the bandwidth keeps the window from the band route (no dense prior, no landmarks kept in the reduced system,
// no lines: the caller says so with `fills`), 0 < m <= COV_BORDER_MAXM, n_b % nb == 0 and n_b > bw' = (hb' + 1) * dpf.
// A landmark's clique costs O(k^2) on its k observers, so only the pairs further apart than hb_lim are enumerated.
#pragma once
#include <algorithm>
#include <utility>
#include <vector>

namespace sadvio {

constexpr int COV_BORDER_MAXM = 96;   // columns of the border: T and T^-1 (2 * 96^2 doubles, 147 KB) fit one workgroup's LDS

// The largest hb the band kernels' LDS image takes ((hb + 1) * dpf + nb <= 128): 19 at dpf 6, 7 at dpf 15
inline int cov_border_hb_max(int dpf) { return dpf == 6 ? 19 : 7; }

enum CovBorderAnswer {
    COV_BORDER_OK = 0,          // borderable: border, core_of, hb_core are the plan
    COV_BORDER_PLAIN,           // no closure edge: the border is empty, the window is the band route's (or the dense route's) as it is
    COV_BORDER_FILLED,          // a dense prior, kept landmarks or lines fill S
    COV_BORDER_TOO_WIDE,        // m > COV_BORDER_MAXM
    COV_BORDER_CORE_SHAPE,      // n_b % nb != 0, or n_b <= bw'
};

// The couplings of a window, by free key-frame index in [0, n_free)
struct CovBorderCouplings {
    int n_free = 0;
    std::vector<int> clique_ptr{0};               // landmark l's observers at clique_kf[clique_ptr[l] .. clique_ptr[l + 1])
    std::vector<int> clique_kf;                   // ascending, distinct
    std::vector<std::pair<int, int>> pairs;       // IMU pairs and relative-pose factors, (lower, higher)
    // One landmark's observing free key-frames, any order, repeats and negative entries (constant key-frames) allowed
    void add_landmark(const int* f, int n) {
        const size_t at = clique_kf.size();
        for (int i = 0; i < n; i++) if (f[i] >= 0) clique_kf.push_back(f[i]);
        std::sort(clique_kf.begin() + at, clique_kf.end());
        clique_kf.erase(std::unique(clique_kf.begin() + at, clique_kf.end()), clique_kf.end());
        if (clique_kf.size() - at < 2) clique_kf.resize(at);
        else clique_ptr.push_back((int)clique_kf.size());
    }
    void add_pair(int a, int b) {
        if (a >= 0 && b >= 0 && a != b) pairs.emplace_back(std::min(a, b), std::max(a, b));
    }
};

struct CovBorderPlan {
    CovBorderAnswer answer = COV_BORDER_PLAIN;
    std::vector<int> border;      // free key-frame indices, ascending
    std::vector<int> core_of;     // [n_free] compacted core index of a free key-frame, -1: in the border
    std::vector<int> order;       // [n_free] free key-frame at position p of [core | border]
    int hb_core = 0;              // hb' of the core in compacted index
    int n_edges = 0;              // distinct closure edges
    int n_core() const { return (int)order.size() - (int)border.size(); }
    bool ok() const { return answer == COV_BORDER_OK; }
};

inline void cov_border_plan(const CovBorderCouplings& Cp, int dpf, int nb, int hb_lim, bool fills, CovBorderPlan& P) {
    const int n = Cp.n_free;
    P.border.clear(); P.core_of.assign((size_t)std::max(n, 0), 0); P.order.clear(); P.hb_core = 0; P.n_edges = 0;
    for (int f = 0; f < n; f++) { P.core_of[f] = f; P.order.push_back(f); }
    if (fills) { P.answer = COV_BORDER_FILLED; return; }
    // 1. closure edges, distinct
    std::vector<std::pair<int, int>> E;
    for (size_t l = 0; l + 1 < Cp.clique_ptr.size(); l++) {
        const int* k = Cp.clique_kf.data() + Cp.clique_ptr[l];
        const int nk = Cp.clique_ptr[l + 1] - Cp.clique_ptr[l];
        if (k[nk - 1] - k[0] <= hb_lim) continue;
        int j = 0;
        for (int i = 0; i < nk; i++) {
            while (j < nk && k[j] - k[i] <= hb_lim) j++;
            for (int q = j; q < nk; q++) E.emplace_back(k[i], k[q]);
        }
    }
    for (const auto& pr : Cp.pairs) if (pr.second - pr.first > hb_lim) E.push_back(pr);
    std::sort(E.begin(), E.end());
    E.erase(std::unique(E.begin(), E.end()), E.end());
    P.n_edges = (int)E.size();
    if (E.empty()) {
        P.answer = COV_BORDER_PLAIN;
    } else {
        // 2. greedy vertex cover
        std::vector<char> covered(E.size(), 0), in_border((size_t)n, 0);
        std::vector<int> deg((size_t)n);
        size_t left = E.size();
        while (left > 0) {
            std::fill(deg.begin(), deg.end(), 0);
            for (size_t e = 0; e < E.size(); e++) if (!covered[e]) { deg[E[e].first]++; deg[E[e].second]++; }
            int best = 0;
            for (int f = 1; f < n; f++) if (deg[f] > deg[best]) best = f;
            in_border[best] = 1;
            for (size_t e = 0; e < E.size(); e++)
                if (!covered[e] && (E[e].first == best || E[e].second == best)) { covered[e] = 1; left--; }
            P.border.push_back(best);
            if ((int)P.border.size() * dpf > COV_BORDER_MAXM) { P.answer = COV_BORDER_TOO_WIDE; break; }
        }
        std::sort(P.border.begin(), P.border.end());
        P.order.clear();
        int c = 0;
        for (int f = 0; f < n; f++) {
            P.core_of[f] = in_border[f] ? -1 : c++;
            if (!in_border[f]) P.order.push_back(f);
        }
        P.order.insert(P.order.end(), P.border.begin(), P.border.end());
        if (P.answer == COV_BORDER_TOO_WIDE) return;
        P.answer = COV_BORDER_OK;
    }
    // 3. hb' of the core: the largest compacted distance a coupling between two core key-frames spans
    for (size_t l = 0; l + 1 < Cp.clique_ptr.size(); l++) {
        int lo = -1, hi = -1;
        for (int q = Cp.clique_ptr[l]; q < Cp.clique_ptr[l + 1]; q++) {
            const int c = P.core_of[Cp.clique_kf[q]];
            if (c >= 0) { if (lo < 0) lo = c; hi = c; }
        }
        if (lo >= 0) P.hb_core = std::max(P.hb_core, hi - lo);
    }
    for (const auto& pr : Cp.pairs) {
        const int a = P.core_of[pr.first], b = P.core_of[pr.second];
        if (a >= 0 && b >= 0) P.hb_core = std::max(P.hb_core, b - a);
    }
    if (P.answer != COV_BORDER_OK) return;
    const int n_b = P.n_core() * dpf, bw = (P.hb_core + 1) * dpf;
    if (n_b % nb != 0 || n_b <= bw) P.answer = COV_BORDER_CORE_SHAPE;
}

}  // namespace sadvio
