// HipOptimizer::set_device_model_gate: landmarkOptimization of the double-sphere map of test_optimizer.cpp's non-pinhole case
// with the chi2 gate on the device (sadvio_ba_landmark_chi2_models) and on the host (host_chi2_gate). Both must flag the same
// landmarks and leave the same positions, with every frame a key-frame (the gate runs on the solved window) and with a frame
// that is none (the gate runs on the re-uploaded all-features window). Exit code 0 = pass. Needs a gfx950 device.
//   test_model_gate                      the check
//   test_model_gate time <calls>         median wall time of one landmarkOptimization, 5 frames x 600 landmarks, the two gates alternating
#include <algorithm>
#include <chrono>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <random>

#include "sadvio_optimizer.hpp"

using namespace sadvio;

static void camera_point(const FrameState& f, const CameraModel& c, const double* p, double* pc) {
    double pf[3];
    for (int a = 0; a < 3; a++) pf[a] = f.T_f_w.R[3 * a] * p[0] + f.T_f_w.R[3 * a + 1] * p[1] + f.T_f_w.R[3 * a + 2] * p[2] + f.T_f_w.t[a];
    for (int a = 0; a < 3; a++) pc[a] = c.T_s_f.R[3 * a] * pf[0] + c.T_s_f.R[3 * a + 1] * pf[1] + c.T_s_f.R[3 * a + 2] * pf[2] + c.T_s_f.t[a];
}

// a stereo double-sphere rig moving along +x, every landmark observed through the model's own projection
static LocalMapSnapshot make_map(std::mt19937& rng, int n_frames, int n_lmk) {
    std::uniform_real_distribution<double> U(-1.0, 1.0);
    LocalMapSnapshot m;
    for (int i = 0; i < n_frames; i++) {
        FrameState f;
        f.id = 100 + i;
        f.T_f_w.t[0] = -0.3 * (n_frames - 1 - i);
        CameraModel c0{350.0, 352.0, 376.0, 240.0, Pose()};
        c0.kind = CameraKind::DoubleSphere; c0.xi = -0.2; c0.alpha = 0.58; c0.width = 752; c0.height = 480;
        CameraModel c1 = c0;
        c1.T_s_f.t[0] = -0.11;
        f.cameras = {c0, c1};
        m.frames.push_back(f);
    }
    while ((int)m.landmarks.size() < n_lmk) {
        LandmarkState L;
        L.id = 5000 + (int64_t)m.landmarks.size();
        L.p[0] = 2.0 * U(rng) + 0.3; L.p[1] = 1.2 * U(rng); L.p[2] = 4.0 + 2.0 * U(rng);
        for (int i = 0; i < n_frames; i++)
            for (int c = 0; c < 2; c++) {
                double pc[3], u, v;
                camera_point(m.frames[i], m.frames[i].cameras[c], L.p, pc);
                if (project_camera(m.frames[i].cameras[c].intrinsics(), pc, u, v) && u > 60 && u < 690 && v > 40 && v < 440) L.features.push_back({i, c, u, v});
            }
        if ((int)L.features.size() >= std::min(4, 2 * n_frames)) m.landmarks.push_back(L);
    }
    return m;
}

static bool same_result(const LocalMapSnapshot& a, const LocalMapSnapshot& b) {
    for (size_t l = 0; l < a.landmarks.size(); l++)
        if (a.landmarks[l].outlier != b.landmarks[l].outlier || std::memcmp(a.landmarks[l].p, b.landmarks[l].p, sizeof(a.landmarks[l].p))) return false;
    return true;
}

int main(int argc, char** argv) {
    std::mt19937 rng(20250404);
    std::normal_distribution<double> G(0.0, 1.0);
    int fails = 0;
    auto check = [&](bool ok, const char* what) { std::printf("%-90s %s\n", what, ok ? "ok" : "FAIL"); if (!ok) fails++; };
    HipOptimizer ang(0, true);

    if (argc > 2 && !std::strcmp(argv[1], "time")) {
        const int calls = std::max(20, std::atoi(argv[2]));
        LocalMapSnapshot m = make_map(rng, 5, 600);
        for (auto& L : m.landmarks) for (double& x : L.p) x += 0.002 * G(rng);
        for (int non_kf = 0; non_kf < 2; non_kf++) {
            m.frames[0].is_keyframe = !non_kf;                       // no key-frame: the gate needs the all-features window uploaded
            std::vector<double> ms[2];
            for (int k = 0; k < 2 * (calls + 5); k++) {              // the two gates alternate: same process, same inputs, same minute
                const int on = k & 1;
                ang.set_device_model_gate(on != 0);
                LocalMapSnapshot c = m;
                const auto t0 = std::chrono::steady_clock::now();
                if (!ang.landmarkOptimization(c)) { std::printf("landmarkOptimization failed: %s\n", ang.last_error().c_str()); return 1; }
                const auto t1 = std::chrono::steady_clock::now();
                if (k >= 10) ms[on].push_back(std::chrono::duration<double, std::milli>(t1 - t0).count());   // 5 warm-up calls each
            }
            for (auto& v : ms) std::sort(v.begin(), v.end());
            std::printf("landmarkOptimization, double-sphere stereo rig, 5 frames x %zu landmarks, %s; %d calls per gate after 5 warm-up calls, alternating: "
                        "host gate median %.3f ms (quartiles %.3f - %.3f), device gate median %.3f ms (quartiles %.3f - %.3f)\n", m.landmarks.size(),
                        non_kf ? "the newest frame no key-frame" : "every frame a key-frame", calls, ms[0][ms[0].size() / 2], ms[0][ms[0].size() / 4],
                        ms[0][3 * ms[0].size() / 4], ms[1][ms[1].size() / 2], ms[1][ms[1].size() / 4], ms[1][3 * ms[1].size() / 4]);
        }
        return 0;
    }

    for (int non_kf = 0; non_kf < 2; non_kf++) {
        LocalMapSnapshot m = make_map(rng, 4, 250);
        m.landmarks[7].p[1] += 0.3;                                  // ~25 px off: fails the gate
        m.landmarks[11].p[2] = -3.0;                                 // behind the rig: every projection fails, 1000 per feature
        for (auto& L : m.landmarks) for (double& x : L.p) x += 0.001 * G(rng);
        if (non_kf) m.frames[0].is_keyframe = false;                 // its features leave the residuals, not the gate
        LocalMapSnapshot host = m, dev = m, again = m;
        ang.set_device_model_gate(false);
        check(ang.landmarkOptimization(host), "landmarkOptimization with the host gate returns true");
        ang.set_device_model_gate(true);
        check(ang.landmarkOptimization(dev), "landmarkOptimization with the device gate returns true");
        ang.set_device_model_gate(false);
        check(ang.landmarkOptimization(again), "landmarkOptimization with the host gate again returns true");
        int n_out = 0, n_moved = 0;
        for (size_t l = 0; l < dev.landmarks.size(); l++) {
            n_out += dev.landmarks[l].outlier;
            n_moved += std::memcmp(dev.landmarks[l].p, m.landmarks[l].p, sizeof(m.landmarks[l].p)) != 0;
        }
        std::printf("   %s: %zu landmarks, %d flagged, %d moved\n", non_kf ? "one frame is no key-frame" : "every frame a key-frame", dev.landmarks.size(), n_out, n_moved);
        check(same_result(host, again), "the host gate is repeatable (the comparison below compares like with like)");
        check(same_result(host, dev), "device gate and host gate: identical outlier flags and landmark positions");
        check(dev.landmarks[7].outlier && dev.landmarks[11].outlier && n_out < 10 && n_moved > 200, "the displaced landmarks are flagged, the others move");
    }
    std::printf(fails ? "FAILED (%d)\n" : "PASSED\n", fails);
    return fails ? 1 : 0;
}
