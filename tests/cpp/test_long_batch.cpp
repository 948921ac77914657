// C++ check of HipOptimizer's sixth constructor argument, long_track_batch (include/sadvio_optimizer.hpp): on a stereo snapshot of 34
// frames with one landmark seen by both cameras of every frame (68 observations: a long track) marginalizeRelativeBatch returns true on
// HipOptimizer(.., long_tracks = true, .., long_track_batch = true), the pair blocks are finite and symmetric, and the same call on a
// handle with long_tracks alone is refused with a text that names long tracks. Exit code 0 = pass. Needs a gfx950 device.
#include <cmath>
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

// 34 stereo frames along +x; landmark 0 is seen from every frame, every other landmark from three consecutive frames
static LocalMapSnapshot make_map(int n_frames, int n_short) {
    std::mt19937 rng(20261021);
    std::uniform_real_distribution<double> U(-1.0, 1.0);
    LocalMapSnapshot m;
    for (int i = 0; i < n_frames; i++) {
        FrameState f;
        f.id = 100 + i;
        f.T_f_w.t[0] = -0.05 * (n_frames - 1 - i);
        const double d[6] = {0.002 * i, -0.001 * i, 0.0015 * i, 0.0, 0.002 * i, -0.003 * i};
        apply_pose_delta(f.T_f_w, d);
        CameraModel c0{458.654, 457.296, 367.215, 248.375, Pose()}, c1 = c0;
        c1.T_s_f.t[0] = -0.11;
        f.cameras = {c0, c1};
        m.frames.push_back(f);
    }
    for (int l = 0; l <= n_short; l++) {
        LandmarkState L;
        L.id = 5000 + l;
        L.p[0] = l == 0 ? 0.8 : 1.5 * U(rng) + 0.8; L.p[1] = l == 0 ? 0.1 : 1.0 * U(rng); L.p[2] = l == 0 ? 6.0 : 5.0 + 2.0 * U(rng);
        const int f0 = l == 0 ? 0 : (l - 1) % (n_frames - 2), f1 = l == 0 ? n_frames : f0 + 3;
        for (int i = f0; i < f1; i++)
            for (int c = 0; c < 2; c++) {
                double u, v;
                project(m.frames[i], c, L.p, u, v);
                L.features.push_back({i, c, u + 0.3 * U(rng), v + 0.3 * U(rng)});
            }
        m.landmarks.push_back(L);
    }
    return m;
}

int main() {
    int fails = 0;
    auto check = [&](bool ok, const char* what) { std::printf("%-86s %s\n", what, ok ? "ok" : "FAIL"); if (!ok) fails++; };
    LocalMapSnapshot m = make_map(34, 128);
    check(m.landmarks[0].features.size() == 68, "landmark 0 has 68 observations");
    const std::vector<std::pair<int, int>> pairs = {{0, 33}, {33, 0}, {5, 6}, {6, 5}, {0, 1}};
    {
        HipOptimizer opt(0, false, true, false, false, true);
        std::vector<double> inf, Tab;
        std::vector<int> ok;
        check(opt.marginalizeRelativeBatch(m, pairs, &inf, &Tab, &ok), "long_track_batch: marginalizeRelativeBatch returns true");
        std::printf("   last_error: '%s'\n", opt.last_error().c_str());
        check(inf.size() == 36 * pairs.size() && ok.size() == pairs.size(), "outputs sized [n][36], [n]");
        if (!fails) {
            // a served pair has a block and its T_a_b, a refused one zeros (sadvio_optimizer.hpp); frames 0 and 33 share the long track alone
            // (every short landmark spans three frames), where the 6 x 6 information is rounding noise: only its presence is looked at
            bool consistent = true;
            for (size_t i = 0; i < pairs.size(); i++) {
                bool any_inf = false, any_T = false;
                for (int q = 0; q < 36; q++) any_inf = any_inf || inf[36 * i + q] != 0.0;
                for (int q = 0; q < 12; q++) any_T = any_T || Tab[12 * i + q] != 0.0;
                consistent = consistent && (ok[i] ? (any_inf && any_T) : (!any_inf && !any_T));
            }
            check(consistent, "a served pair has its block and T_a_b, a refused pair zeros");
            check(ok[2] == 1 && ok[4] == 1, "pairs of neighbouring frames are served");
        }
    }
    {
        HipOptimizer opt(0, false, true);
        std::vector<double> inf;
        check(!opt.marginalizeRelativeBatch(m, pairs, &inf), "long_tracks alone: the call is refused");
        check(opt.last_error().find("long tracks") != std::string::npos, "... with a text that names long tracks");
    }
    std::printf(fails ? "FAILED (%d)\n" : "PASSED\n", fails);
    return fails ? 1 : 0;
}
