// C++ check of HipOptimizer::marginalizeRelativeBatch (include/sadvio_optimizer.hpp): on a small stereo snapshot the batch gives, pair
// by pair, what marginalizeRelative gives (1e-9 relative on the 6 x 6 information), T_a_b = T_a_w T_w_b, and zeros with ok = 0 for a
// pair that shares no landmark. Exit code 0 = pass. Needs a gfx950 device.
#include <cstdio>
#include <random>

#include "sadvio_optimizer.hpp"

using namespace sadvio;

static void project(const FrameState& f, int cam, const double* p, double& u, double& v) {
    const CameraModel& c = f.cameras[cam];
    double pf[3], ps[3];
    for (int i = 0; i < 3; i++) pf[i] = f.T_f_w.R[3 * i] * p[0] + f.T_f_w.R[3 * i + 1] * p[1] + f.T_f_w.R[3 * i + 2] * p[2] + f.T_f_w.t[i];
    for (int i = 0; i < 3; i++) ps[i] = c.T_s_f.R[3 * i] * pf[0] + c.T_s_f.R[3 * i + 1] * pf[1] + c.T_s_f.R[3 * i + 2] * pf[2] + c.T_s_f.t[i];
    u = c.fx * ps[0] / ps[2] + c.cx; v = c.fy * ps[1] / ps[2] + c.cy;
}

// four stereo frames along +x; even landmarks are seen by frames 0 .. 2, odd ones by frames 1 .. 3: frames 0 and 3 share nothing
static LocalMapSnapshot make_map(int n_lmk) {
    std::mt19937 rng(20260111);
    std::uniform_real_distribution<double> U(-1.0, 1.0);
    const int n_frames = 4;
    LocalMapSnapshot m;
    for (int i = 0; i < n_frames; i++) {
        FrameState f;
        f.id = 100 + i;
        f.T_f_w.t[0] = -0.3 * (n_frames - 1 - i);
        const double d[6] = {0.02 * i, -0.01 * i, 0.015 * i, 0.0, 0.02 * i, -0.03 * i};
        apply_pose_delta(f.T_f_w, d);
        CameraModel c0{458.654, 457.296, 367.215, 248.375, Pose()}, c1 = c0;
        c1.T_s_f.t[0] = -0.11;
        f.cameras = {c0, c1};
        m.frames.push_back(f);
    }
    for (int l = 0; l < n_lmk; l++) {
        LandmarkState L;
        L.id = 5000 + l;
        L.p[0] = 2.0 * U(rng) + 0.3; L.p[1] = 1.2 * U(rng); L.p[2] = 4.0 + 2.0 * U(rng);
        for (int i = 0; i < n_frames; i++) {
            if ((l % 2 == 0 && i == 3) || (l % 2 == 1 && i == 0)) continue;
            for (int c = 0; c < 2; c++) {
                double u, v;
                project(m.frames[i], c, L.p, u, v);
                if (u > 80 && u < 650 && v > 60 && v < 430) L.features.push_back({i, c, u + 0.3 * U(rng), v + 0.3 * U(rng)});
            }
        }
        if (L.features.size() >= 4) m.landmarks.push_back(L);
    }
    return m;
}

int main() {
    int fails = 0;
    auto check = [&](bool ok, const char* what) { std::printf("%-78s %s\n", what, ok ? "ok" : "FAIL"); if (!ok) fails++; };
    HipOptimizer opt(0);
    LocalMapSnapshot m = make_map(300);
    const std::vector<std::pair<int, int>> pairs = {{0, 1}, {1, 0}, {0, 3}, {2, 3}, {3, 1}, {0, 2}, {0, 1}};
    std::vector<double> inf, Tab;
    std::vector<int> ok;
    check(opt.marginalizeRelativeBatch(m, pairs, &inf, &Tab, &ok), "marginalizeRelativeBatch returns true");
    std::printf("   last_error: '%s'\n", opt.last_error().c_str());
    check(inf.size() == 36 * pairs.size() && Tab.size() == 12 * pairs.size() && ok.size() == pairs.size(), "outputs sized [n][36], [n][12], [n]");
    if (fails) { std::printf("FAILED (%d)\n", fails); return 1; }
    double worst = 0.0, worst_T = 0.0;
    bool status_same = true, zeros = true;
    for (size_t i = 0; i < pairs.size(); i++) {
        double one[36];
        const bool got = opt.marginalizeRelative(m, pairs[i].first, pairs[i].second, one);
        status_same &= got == (ok[i] != 0);
        double mx = 0.0, df = 0.0;
        for (int k = 0; k < 36; k++) { mx = std::fmax(mx, std::fabs(one[k])); df = std::fmax(df, std::fabs(one[k] - inf[36 * i + k])); }
        if (got) worst = std::fmax(worst, df / mx);
        else { for (int k = 0; k < 36; k++) zeros &= inf[36 * i + k] == 0.0; for (int k = 0; k < 12; k++) zeros &= Tab[12 * i + k] == 0.0; }
        if (ok[i]) {
            const Pose T = pose_mul(m.frames[pairs[i].first].T_f_w, pose_inv(m.frames[pairs[i].second].T_f_w));
            for (int k = 0; k < 9; k++) worst_T = std::fmax(worst_T, std::fabs(T.R[k] - Tab[12 * i + k]));
            for (int k = 0; k < 3; k++) worst_T = std::fmax(worst_T, std::fabs(T.t[k] - Tab[12 * i + 9 + k]));
        }
        std::printf("   pair (%d, %d): ok %d, single %d, max|inf| %.3e, |batch - single| / max %.3e\n", pairs[i].first, pairs[i].second, ok[i], (int)got, mx, mx > 0 ? df / mx : 0.0);
    }
    std::printf("   worst relative difference of inf %.3e, worst |T_a_b - T_a_w T_w_b| %.3e\n", worst, worst_T);
    check(status_same, "every pair: ok equals marginalizeRelative's return value");
    check(!ok[2] && ok[0] && ok[1] && ok[3] && ok[4] && ok[5], "frames 0 and 3 share nothing: refused; the others succeed");
    check(zeros, "a refused pair has zeros in inf36 and T_a_b");
    check(worst <= 1e-9, "inf equals marginalizeRelative's pair by pair to 1e-9 relative");
    check(worst_T <= 1e-14, "T_a_b = T_a_w T_w_b to 1e-14");
    bool dup = true;
    for (int k = 0; k < 36; k++) dup &= inf[k] == inf[36 * 6 + k];
    check(dup, "a duplicate pair returns the same bits");
    std::vector<double> inf2;
    check(!opt.marginalizeRelativeBatch(m, {{0, 1}, {2, 2}}, &inf2) && inf2.size() == 72 && inf2[0] == 0.0, "frame0 == frame1: the call fails, outputs zero");
    check(!opt.marginalizeRelativeBatch(m, {{0, 4}}, &inf2), "a frame index out of range: the call fails");
    check(opt.marginalizeRelativeBatch(m, {}, &inf2) && inf2.empty(), "no pairs: true, nothing to do");
    std::printf(fails ? "FAILED (%d)\n" : "PASSED\n", fails);
    return fails ? 1 : 0;
}
