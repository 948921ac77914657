// CPU check of nofov_flatten (include/sadvio_optimizer.hpp): the landmark selection of
// AngularAdjustmentCERESAnalytic::landmarkOptimizationNoFov (AngularAdjustmentCERESAnalytic.cpp:775-851). No device needed:
// the program links against nothing but the header's inline code. Exit code 0 = pass.
#include <cstdio>

#include "sadvio_optimizer.hpp"

using namespace sadvio;

int main() {
    int fails = 0;
    auto check = [&](bool ok, const char* what) { std::printf("%-70s %s\n", what, ok ? "ok" : "FAIL"); if (!ok) fails++; };
    LocalMapSnapshot m;
    for (int k = 0; k < 4; k++) {                        // 0 = fp, 1 = f, 2 = key-frame, 3 = not a key-frame
        FrameState f;
        f.id = k;
        f.T_f_w.t[0] = 0.1 * k;
        CameraModel c0{100, 100, 400, 400, Pose()}, c1 = c0;
        c1.fx = c1.fy = 200;
        c1.T_s_f.t[1] = 0.2;
        f.cameras = {c0, c1};
        m.frames.push_back(f);
    }
    m.frames[1].cameras[0].fx = 120; m.frames[1].cameras[0].fy = 80;   // gate = 2 / 100
    m.frames[3].is_keyframe = false;
    auto lmk = [&](std::vector<Feature> fs) { LandmarkState L; L.id = (int64_t)m.landmarks.size(); L.p[2] = 5; L.features = fs; m.landmarks.push_back(L); };
    lmk({{1, 0, 400, 400}, {0, 1, 410, 400}});                         // 0: plain
    lmk({{1, 0, 400, 400}, {1, 1, 300, 420}, {0, 0, 390, 400}, {0, 1, 420, 380}, {2, 0, 401, 401}, {3, 0, 402, 402}});   // 1: last wins, feats, non-KF
    lmk({{1, 0, 400, 400}, {3, 1, 400, 400}});                         // 2: featp only on a non-key-frame -> dropped
    lmk({{0, 0, 400, 400}, {2, 0, 400, 400}});                         // 3: no feat -> dropped
    lmk({{1, 0, 400, 400}, {0, 0, 400, 400}});                         // 4: outlier
    m.landmarks.back().outlier = true;
    lmk({{1, 0, 400, 400}, {0, 0, 400, 400}});                         // 5: not initialised
    m.landmarks.back().initialized = false;
    lmk({{1, 0, 400, 400}, {0, 0, 400, 400}, {7, 0, 1, 1}, {2, 5, 1, 1}});   // 6: features of missing frames / sensors ignored
    Pose Tm;
    Tm.t[0] = 0.5;
    NoFovFlat F;
    check(nofov_flatten(m, 1, 0, Tm, 3.0, F), "nofov_flatten accepts the snapshot");
    check(F.lmk_src == std::vector<int>({0, 1, 6}), "selection: initialised inliers with feat and featp only");
    check(F.pb.n_lmk == 3 && F.ptr == std::vector<int32_t>({0, 1, 3, 4}), "CSR: f's factor, then the key-frame feats");
    check(F.frame_src == std::vector<int>({1, 2}), "problem frames: f first, non-key-frames never");
    check(F.obs_frame == std::vector<int32_t>({0, 0, 1, 0}), "observation frames");
    // landmark 1: feat is the last feature on f (sensor 1), featp the last on fp (sensor 1)
    check(F.cam_frame[F.obs_cam[1]] == 1 && F.cam_sensor[F.obs_cam[1]] == 1, "the last feature on f wins");
    check(F.cam_frame[F.scale_cam[1]] == 0 && F.cam_sensor[F.scale_cam[1]] == 1, "the last feature on fp wins");
    check(F.cam_frame[0] == 1 && F.cam_sensor[0] == 0 && F.pb.cam0 == 0, "cam0 is f's sensor 0");
    double b[3];
    ray_camera(m.frames[0].cameras[1].intrinsics(), 420, 380, b);
    check(std::fabs(F.scale_bearing[3] - b[0]) < 1e-15 && std::fabs(F.scale_bearing[5] - b[2]) < 1e-15, "featp's bearing from its camera model");
    check(std::fabs(F.gate - 0.02) < 1e-15 && F.pb.gate == F.gate && F.pb.info_scale == 3.0, "gate = 2 / focal of f's sensor 0");
    check(F.pb.T_cam0_cam0p[9] == 0.5 && F.pb.n_obs == 4 && F.pb.n_frames == 2 && F.pb.n_cam == (int)F.cam_frame.size(), "problem header");
    check(F.pb.lmk_obs_ptr == F.ptr.data() && F.pb.obs_bearing == F.obs_bearing.data(), "problem points into the flat arrays");
    check(!nofov_flatten(m, 1, 1, Tm, 0.0, F) && !nofov_flatten(m, 9, 0, Tm, 0.0, F), "bad frame indices are refused");
    std::printf(fails ? "FAILED (%d)\n" : "PASSED\n", fails);
    return fails ? 1 : 0;
}
