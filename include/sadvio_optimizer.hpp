// sadvio_optimizer.hpp — C++17 host layer over the C ABI (include/sadvio_ba.h), header-only, no third-party types.
//
// Mirrors the solve entry points of isae::AOptimizer (cpp/include/isaeslam/optimizers/AOptimizer.h:22-45) — same
// names, same argument meaning, same return convention — on a plain-struct snapshot of what those methods read from
// isae::LocalMap / isae::Frame / isae::ALandmark. The reference's own classes need Eigen / Ceres / OpenCV (absent in
// this image); the adapter of INTEGRATION.md fills these structs from them and copies the results back.
// Everything the reference does around ceres::Solve is here: the inclusion rules of addResidualsLocalMap
// (BundleAdjustmentCERESAnalytic.cpp:197-314), the solver options of each entry point and the write-back
// (AOptimizer.cpp:329-340, 391-434).
#pragma once
#include <algorithm>
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <stdexcept>
#include <array>
#include <string>
#include <utility>
#include <vector>

#include "sadvio_ba.h"
#include "sadvio_cameras.hpp"
#include "sadvio_io.hpp"

namespace sadvio {

struct Pose {                 // Eigen::Affine3d as 3x3 row-major + translation
    double R[9] = {1, 0, 0, 0, 1, 0, 0, 0, 1};
    double t[3] = {0, 0, 0};
};

inline void exp_so3(const double* w, double* R) {   // geometry.h:131-147 (first order below 1e-9)
    const double a = std::sqrt(w[0] * w[0] + w[1] * w[1] + w[2] * w[2]);
    const double I[9] = {1, 0, 0, 0, 1, 0, 0, 0, 1};
    if (a < 1e-9) {
        const double S[9] = {0, -w[2], w[1], w[2], 0, -w[0], -w[1], w[0], 0};
        for (int i = 0; i < 9; i++) R[i] = I[i] + S[i];
        return;
    }
    const double x = w[0] / a, y = w[1] / a, z = w[2] / a;
    const double S[9] = {0, -z, y, z, 0, -x, -y, x, 0};
    double S2[9];
    for (int i = 0; i < 3; i++)
        for (int j = 0; j < 3; j++) S2[3 * i + j] = S[3 * i] * S[j] + S[3 * i + 1] * S[3 + j] + S[3 * i + 2] * S[6 + j];
    for (int i = 0; i < 9; i++) R[i] = I[i] + (1.0 - std::cos(a)) * S2[i] + std::sin(a) * S[i];
}

// T <- T * (exp(w), t): frame write-back (AOptimizer.cpp:329-332, parametersBlock.hpp:34-37)
inline void apply_pose_delta(Pose& T, const double* d6) {
    double dR[9], R[9], t[3];
    exp_so3(d6, dR);
    for (int i = 0; i < 3; i++) {
        for (int j = 0; j < 3; j++) R[3 * i + j] = T.R[3 * i] * dR[j] + T.R[3 * i + 1] * dR[3 + j] + T.R[3 * i + 2] * dR[6 + j];
        t[i] = T.R[3 * i] * d6[3] + T.R[3 * i + 1] * d6[4] + T.R[3 * i + 2] * d6[5] + T.t[i];
    }
    std::memcpy(T.R, R, sizeof(R)); std::memcpy(T.t, t, sizeof(t));
}

// IMU::biasDeltaCorrection (IMU.cpp:104-108): first-order update of a pre-integration for a bias change of its older frame
inline void bias_delta_correction(sadvio_imu_factor& f, const double* d_ba, const double* d_bg) {
    double w[3], E[9], R[9];
    for (int i = 0; i < 3; i++) {
        double dp = 0, dv = 0; w[i] = 0;
        for (int j = 0; j < 3; j++) {
            dp += f.J_dp_ba[3 * i + j] * d_ba[j] + f.J_dp_bg[3 * i + j] * d_bg[j];
            dv += f.J_dv_ba[3 * i + j] * d_ba[j] + f.J_dv_bg[3 * i + j] * d_bg[j];
            w[i] += f.J_dR_bg[3 * i + j] * d_bg[j];
        }
        f.delta_p[i] += dp; f.delta_v[i] += dv;
    }
    exp_so3(w, E);
    for (int i = 0; i < 3; i++)
        for (int j = 0; j < 3; j++) R[3 * i + j] = f.delta_R[3 * i] * E[j] + f.delta_R[3 * i + 1] * E[3 + j] + f.delta_R[3 * i + 2] * E[6 + j];
    std::memcpy(f.delta_R, R, sizeof(R));
}

struct CameraModel {          // one ImageSensor of a key-frame: K + frame -> sensor transform (+ the model's parameters)
    double fx, fy, cx, cy;
    Pose T_s_f;
    double width = 0, height = 0;   // image size used by ALandmark::sanityCheck (Camera.cpp:45); 0 = (2 cx, 2 cy)
    // non-pinhole models (sadvio_cameras.hpp) only work with the ANGULAR backend, as in the reference: the bearing comes
    // from the model's getRayCamera, the factor itself is model-free
    CameraKind kind = CameraKind::Pinhole;
    double rmax = 1, xi = 0, alpha = 0;
    bool distortion = false;
    double D[4] = {0, 0, 0, 0};
    CameraIntrinsics intrinsics() const {
        CameraIntrinsics k;
        k.kind = kind; k.fx = fx; k.fy = fy; k.cx = cx; k.cy = cy; k.rmax = rmax; k.xi = xi; k.alpha = alpha; k.distortion = distortion;
        for (int i = 0; i < 4; i++) k.D[i] = D[i];
        k.width = width > 0 ? width : 2.0 * cx; k.height = height > 0 ? height : 2.0 * cy;
        return k;
    }
};

struct FrameState {           // what the optimizer reads / writes of an isae::Frame (+ its IMU)
    int64_t id = 0;
    Pose T_f_w;
    bool is_keyframe = true;  // Frame::isKeyFrame: window / landmark solves only use features of key-frames (…Analytic.cpp:131,256)
    std::vector<CameraModel> cameras;
    bool has_prior = false;   // Frame::hasPrior / getPrior / getInfPrior (…Analytic.cpp:224-228)
    Pose T_prior;
    double inf_prior[6] = {0, 0, 0, 0, 0, 0};
    bool has_imu = false;
    double v[3] = {0, 0, 0}, ba[3] = {0, 0, 0}, bg[3] = {0, 0, 0};
    sadvio_imu_factor preint{};   // pre-integration towards the NEXT OLDER... see LocalMapSnapshot::imu_pairs
};

struct Feature {              // one AFeature of a landmark: which frame / camera saw it where
    int frame;                // index into LocalMapSnapshot::frames
    int camera;               // index into that frame's cameras
    double u, v;              // pixel measurement (pixel factor) — bearings are derived (Camera.cpp:15-25)
};

struct LandmarkState {
    int64_t id = 0;
    double p[3] = {0, 0, 0};  // T_w_l translation
    bool initialized = true, outlier = false;
    bool in_map = true;       // ALandmark::isInMap
    bool has_prior = false;   // ALandmark::hasPrior / setPrior (set by marginalize, marginalization.cpp:83)
    std::vector<Feature> features;
};

struct LineFeature {          // one AFeature of a linexd landmark: the two end points of the 2D segment (AFeature::getPoints)
    int frame, camera;
    double u0, v0, u1, v1;
};

struct LineLandmarkState {    // a "linexd" landmark: pose T_w_l whose x axis carries the segment (Line3D.h)
    int64_t id = 0;
    Pose T_w_l;
    double model[6] = {-0.5, 0, 0, 0.5, 0, 0};   // ModelLine3D end points as ReprojectionErrCeres_linexd_dx reads them: model3d_->getModel(), getScale() NOT applied
                                                 // (BundleAdjustmentCERESAnalytic.h:128,165; Line3D multiplies _scale by 100, Line3D.h:15, but the BA residual never reads it)
    bool initialized = true, outlier = false;
    std::vector<LineFeature> features;
};

struct ImuPair {              // IMUFactor + IMUBiasFactor between two consecutive key-frames (AOptimizer.cpp:55-92)
    int frame_i, frame_j;     // i = older
    sadvio_imu_factor f;      // kf_i / kf_j are filled by the optimizer
};

struct LocalMapSnapshot {     // LocalMap::getLastNFramesIn (newest first, amap.h:28-32) + getLandmarks()["pointxd"]
    std::vector<FrameState> frames;
    std::vector<LandmarkState> landmarks;
    std::vector<ImuPair> imu_pairs;
    std::vector<LineLandmarkState> lines;   // getLandmarks()["linexd"]
};

inline Pose pose_mul(const Pose& a, const Pose& b) {   // a * b
    Pose c;
    for (int i = 0; i < 3; i++) {
        for (int j = 0; j < 3; j++) c.R[3 * i + j] = a.R[3 * i] * b.R[j] + a.R[3 * i + 1] * b.R[3 + j] + a.R[3 * i + 2] * b.R[6 + j];
        c.t[i] = a.R[3 * i] * b.t[0] + a.R[3 * i + 1] * b.t[1] + a.R[3 * i + 2] * b.t[2] + a.t[i];
    }
    return c;
}
inline Pose pose_inv(const Pose& a) {
    Pose c;
    for (int i = 0; i < 3; i++) for (int j = 0; j < 3; j++) c.R[3 * i + j] = a.R[3 * j + i];
    for (int i = 0; i < 3; i++) c.t[i] = -(c.R[3 * i] * a.t[0] + c.R[3 * i + 1] * a.t[1] + c.R[3 * i + 2] * a.t[2]);
    return c;
}

// Covariance of a key-frame's pose for a consumer that speaks T_w_f (a ROS odometry message: geometry_msgs/PoseWithCovariance,
// parameters in the order x, y, z, rotation about the fixed X, Y, Z axes). The library's 6 x 6 block (sadvio_ba_covariance) is over
// the delta coordinates (w, tau) of T_f_w, composed on the right (geometry.h:198-203; parametersBlock.hpp:34-37):
//     T_f_w' = T_f_w (exp(w), tau):   R' = R exp(w),   t' = R tau + t.
// With T_w_f = T_f_w^-1 = (Q, c), Q = R^T, c = -R^T t, the same perturbation reads
//     Q' = exp(w)^T R^T = exp(-w) Q,          c' = -Q' t' = -exp(-w) (tau + R^T t) = exp(-w) (c - tau).
// Orientation error about the fixed (world) axes, Q' = exp(theta) Q:  theta = -w (exactly). Position error in the world:
//     dc = c' - c = exp(-w) (c - tau) - c = [c]x w - tau + O(2)        (exp(-w) c = c - w x c = c + [c]x w to first order).
// So (dc, theta) = Jm (w, tau) with  Jm = [ [c]x  -I ; -I  0 ]  and  cov_ros = Jm cov_wt Jm^T. cov_wt36 and cov_ros36 are row-major
// and may not alias. T_f_w is the key-frame's pose AFTER the solve's write-back (the state the covariance was evaluated at).
inline void pose_covariance_jacobian(const Pose& T_f_w, double* Jm36) {
    const Pose T_w_f = pose_inv(T_f_w);
    const double* c = T_w_f.t;
    const double Cx[9] = {0, -c[2], c[1], c[2], 0, -c[0], -c[1], c[0], 0};
    for (int i = 0; i < 36; i++) Jm36[i] = 0.0;
    for (int i = 0; i < 3; i++) {
        for (int j = 0; j < 3; j++) Jm36[6 * i + j] = Cx[3 * i + j];
        Jm36[6 * i + 3 + i] = -1.0;
        Jm36[6 * (3 + i) + i] = -1.0;
    }
}
inline void pose_covariance_ros(const Pose& T_f_w, const double* cov_wt36, double* cov_ros36) {
    double Jm[36], T[36];
    pose_covariance_jacobian(T_f_w, Jm);
    for (int i = 0; i < 6; i++)
        for (int j = 0; j < 6; j++) {
            double v = 0.0;
            for (int k = 0; k < 6; k++) v += Jm[6 * i + k] * cov_wt36[6 * k + j];
            T[6 * i + j] = v;
        }
    for (int i = 0; i < 6; i++)
        for (int j = 0; j < 6; j++) {
            double v = 0.0;
            for (int k = 0; k < 6; k++) v += T[6 * i + k] * Jm[6 * j + k];
            cov_ros36[6 * i + j] = v;
        }
}

// The 95 % gate on a squared Mahalanobis distance (HipOptimizer::covarianceCross: maha2 of a candidate observation, dof = 2): true
// when maha2 is at most the chi-square quantile of `dof` degrees of freedom (1: 3.841, 2: 5.991, 3: 7.815; any other dof: false).
// A NaN (singular landmark) never passes.
inline bool innovation_gate(double maha2, int dof = 2) {
    const double q95[4] = {0.0, 3.841458820694124, 5.991464547107979, 7.814727903251179};
    return dof >= 1 && dof <= 3 && maha2 >= 0.0 && maha2 <= q95[dof];
}

// The problem of AngularAdjustmentCERESAnalytic::landmarkOptimizationNoFov (AngularAdjustmentCERESAnalytic.cpp:775-851) in the
// layout of sadvio_nofov_problem. Selection: a landmark that is initialised and not an outlier (:778); of its features, only
// those of key-frames count (:788); the one on f is `feat`, the one on fp is `featp` (the last one wins, :792-800), every other
// one goes to `feats` (:802); the landmark enters only with both feat and featp (:806). Problem frame 0 is f, the others
// follow in order of first use; cameras are (frame, sensor) pairs in order of first use, f's sensor 0 first. Bearings come
// from each camera model (getRayCamera). A feature whose frame or sensor does not exist is ignored.
struct NoFovFlat {
    std::vector<double> frame_T, cam_T, lmk_p, scale_bearing, obs_bearing;
    std::vector<int32_t> scale_cam, ptr{0}, obs_frame, obs_cam;
    std::vector<int> lmk_src;     // snapshot landmark of each problem landmark
    std::vector<int> frame_src;   // snapshot frame of each problem frame (frame_src[0] = f)
    std::vector<int> cam_frame, cam_sensor;
    double gate = 0.0;            // 2 / focal of f's sensor 0 (:890, Camera.h:46)
    double T_cam0_cam0p[12] = {};
    sadvio_nofov_problem pb{};    // points into the members above: fill in place, do not copy
};

inline bool nofov_flatten(const LocalMapSnapshot& map, int f, int fp, const Pose& T_cam0_cam0p, double info_scale, NoFovFlat& F) {
    const int nf = (int)map.frames.size();
    F = NoFovFlat();
    if (f < 0 || f >= nf || fp < 0 || fp >= nf || f == fp || map.frames[f].cameras.empty()) return false;
    std::vector<int> frame_of(nf, -1);
    std::vector<std::vector<int>> cam_of(nf);
    for (int k = 0; k < nf; k++) cam_of[k].assign(map.frames[k].cameras.size(), -1);
    auto frame_idx = [&](int k) {
        if (frame_of[k] < 0) {
            frame_of[k] = (int)F.frame_src.size(); F.frame_src.push_back(k);
            F.frame_T.insert(F.frame_T.end(), map.frames[k].T_f_w.R, map.frames[k].T_f_w.R + 9);
            F.frame_T.insert(F.frame_T.end(), map.frames[k].T_f_w.t, map.frames[k].T_f_w.t + 3);
        }
        return frame_of[k];
    };
    auto cam_idx = [&](int k, int c) {
        if (cam_of[k][c] < 0) {
            const Pose& T = map.frames[k].cameras[c].T_s_f;
            cam_of[k][c] = (int)F.cam_frame.size(); F.cam_frame.push_back(k); F.cam_sensor.push_back(c);
            F.cam_T.insert(F.cam_T.end(), T.R, T.R + 9); F.cam_T.insert(F.cam_T.end(), T.t, T.t + 3);
        }
        return cam_of[k][c];
    };
    auto bearing = [&](const Feature& ft, std::vector<double>& out) {
        double b[3] = {0.0, 0.0, 1.0};
        ray_camera(map.frames[ft.frame].cameras[ft.camera].intrinsics(), ft.u, ft.v, b);
        out.insert(out.end(), {b[0], b[1], b[2]});
    };
    frame_idx(f);
    cam_idx(f, 0);
    const CameraModel& c0 = map.frames[f].cameras[0];
    F.gate = 2.0 / ((c0.fx + c0.fy) / 2.0);
    for (int l = 0; l < (int)map.landmarks.size(); l++) {
        const LandmarkState& L = map.landmarks[l];
        if (!L.initialized || L.outlier) continue;                                        // :778-779
        const Feature* feat = nullptr; const Feature* featp = nullptr;
        std::vector<const Feature*> feats;
        for (const Feature& ft : L.features) {
            if (ft.frame < 0 || ft.frame >= nf || ft.camera < 0 || ft.camera >= (int)map.frames[ft.frame].cameras.size()) continue;
            if (!map.frames[ft.frame].is_keyframe) continue;                              // :788-790
            if (ft.frame == f) feat = &ft;                                                // :792-795
            else if (ft.frame == fp) featp = &ft;                                         // :797-800
            else feats.push_back(&ft);                                                    // :802
        }
        if (!feat || !featp) continue;                                                    // :806
        F.lmk_src.push_back(l);
        F.lmk_p.insert(F.lmk_p.end(), L.p, L.p + 3);
        bearing(*featp, F.scale_bearing);
        F.scale_cam.push_back(cam_idx(featp->frame, featp->camera));
        for (const Feature* ft : {feat}) {                                                // f's factor first (:819-831), then feats (:833-849)
            F.obs_frame.push_back(frame_idx(ft->frame)); F.obs_cam.push_back(cam_idx(ft->frame, ft->camera)); bearing(*ft, F.obs_bearing);
        }
        for (const Feature* ft : feats) {
            F.obs_frame.push_back(frame_idx(ft->frame)); F.obs_cam.push_back(cam_idx(ft->frame, ft->camera)); bearing(*ft, F.obs_bearing);
        }
        F.ptr.push_back((int32_t)F.obs_frame.size());
    }
    sadvio_nofov_problem& p = F.pb;
    p.n_lmk = (int32_t)F.lmk_src.size(); p.n_obs = (int32_t)F.obs_frame.size(); p.n_frames = (int32_t)F.frame_src.size();
    p.n_cam = (int32_t)F.cam_frame.size(); p.cam0 = 0; p.fix_scale = -1;
    p.frame_T_f_w = F.frame_T.data(); p.cam_T_s_f = F.cam_T.data();
    std::memcpy(F.T_cam0_cam0p, T_cam0_cam0p.R, 72); std::memcpy(F.T_cam0_cam0p + 9, T_cam0_cam0p.t, 24);
    p.T_cam0_cam0p = F.T_cam0_cam0p;
    p.info_scale = info_scale; p.gate = F.gate;
    p.lmk_p = F.lmk_p.data(); p.scale_bearing = F.scale_bearing.data(); p.scale_cam = F.scale_cam.data();
    p.lmk_obs_ptr = F.ptr.data(); p.obs_frame = F.obs_frame.data(); p.obs_cam = F.obs_cam.data(); p.obs_bearing = F.obs_bearing.data();
    return true;
}

class HipOptimizer {
  public:
    // long_tracks: landmarks with more than 64 observations are accepted (SADVIO_CFG_LONG_TRACKS, sadvio_ba.h); such a window is
    // marginalised, sparsified and given priors on its long tracks only with long_track_priors (SADVIO_CFG_LONG_TRACK_PRIORS), and asked
    // for covariances (covariance(), covarianceCross(); not the batch call) only with long_track_covariance
    // (SADVIO_CFG_LONG_TRACK_COVARIANCE). Both need long_tracks and are independent of each other. long_track_batch
    // (SADVIO_CFG_LONG_TRACK_BATCH, needs long_tracks): marginalizeRelative() and marginalizeRelativeBatch() serve such a window, and
    // with long_track_covariance the batch covariance call does
    explicit HipOptimizer(int device = 0, bool angular = false, bool long_tracks = false, bool long_track_priors = false,
                          bool long_track_covariance = false, bool long_track_batch = false) : _angular(angular) {
        sadvio_ba_config cfg{device, 0, 1, (long_tracks ? SADVIO_CFG_LONG_TRACKS : 0) | (long_track_priors ? SADVIO_CFG_LONG_TRACK_PRIORS : 0) |
                                               (long_track_covariance ? SADVIO_CFG_LONG_TRACK_COVARIANCE : 0) |
                                               (long_track_batch ? SADVIO_CFG_LONG_TRACK_BATCH : 0)};
        const int rc = sadvio_ba_create(&cfg, &_h);
        if (rc == SADVIO_E_INVALID_ARG) throw std::runtime_error(std::string("sadvio: ") + sadvio_ba_last_error(nullptr));
        if (rc != SADVIO_OK) throw std::runtime_error("sadvio: no usable gfx950 device");
    }
    ~HipOptimizer() { sadvio_ba_destroy(_h); }
    HipOptimizer(const HipOptimizer&) = delete;
    HipOptimizer& operator=(const HipOptimizer&) = delete;

    // AOptimizer::localMapBA (AOptimizer.cpp:299-350): always returns true; on a backend error the state is untouched.
    bool localMapBA(LocalMapSnapshot& map, size_t fixed_frame_number = 0) {
        sadvio_solve_options o; sadvio_ba_default_options(&o);           // LM, 20 iterations, f_tol 1e-3 (:315-323)
        solve(map, fixed_frame_number, false, o, /*all_frames_const*/ false, /*landmarks_const*/ false);
        return true;
    }
    // AOptimizer::localMapVIOptimization (:352-446)
    bool localMapVIOptimization(LocalMapSnapshot& map, size_t fixed_frame_number = 0) {
        sadvio_solve_options o; sadvio_ba_default_options(&o);
        solve(map, fixed_frame_number, true, o, false, false);
        return true;
    }
    // AOptimizer::landmarkOptimization (:98-150): poses constant, Huber(sqrt(1.345)), 10 iterations; a landmark is
    // written back only if it passes ALandmark::sanityCheck — evaluated, as in the reference, at the pose it had BEFORE
    // the solve (:124-141) — and is flagged outlier / inlier by that check
    bool landmarkOptimization(LocalMapSnapshot& map) {
        sadvio_solve_options o; sadvio_ba_default_options(&o);
        o.max_num_iterations = 10; o.huber_a = std::sqrt(1.345);
        solve(map, 0, false, o, true, false, true);
        return true;
    }
    // AOptimizer::singleFrameOptimization (:152-217): frame 0 free, landmarks constant, 5 iterations, no loss
    bool singleFrameOptimization(LocalMapSnapshot& map) {
        sadvio_solve_options o; sadvio_ba_default_options(&o);
        o.max_num_iterations = 5;
        solve(map, 0, false, o, false, true);
        return true;
    }
    // AOptimizer::singleFrameVIOptimization (:219-297): returns summary.IsSolutionUsable()
    bool singleFrameVIOptimization(LocalMapSnapshot& map) {
        sadvio_solve_options o; sadvio_ba_default_options(&o);
        o.max_num_iterations = 5; o.huber_a = std::sqrt(1.345);
        o.max_solver_time_in_seconds = 0.005;                                            // :254
        return solve(map, 0, true, o, false, true);
    }

    // AOptimizer::VIInit (:448-581): gravity direction, velocities and (optim_scale) the metric scale of a visual-only
    // map from the pre-integrated IMU factors between its key-frames; returns exp(lambda) and applies the result as
    // :526-562 — velocities += dv, T_f_w <- (R_f_w, s t_f_w) * (R_w_i, 0), priors re-anchored at 100, landmarks
    // p <- s R_w_i^T p. (The reference adds dba to Ba twice and never updates Bg, :529-530; both deltas are constant
    // zero in this problem, :472-476, so nothing is written.) R_w_i is row-major 3x3. On a backend error nothing is
    // written and 1.0 is returned.
    double VIInit(LocalMapSnapshot& map, double* R_w_i, bool optim_scale = false) {
        const int n = (int)map.frames.size();
        std::vector<double> T(12 * (size_t)n), vel(3 * (size_t)n), dv(3 * (size_t)n, 0.0);
        for (int i = 0; i < n; i++) {
            std::memcpy(&T[12 * (size_t)i], map.frames[i].T_f_w.R, 72); std::memcpy(&T[12 * (size_t)i + 9], map.frames[i].T_f_w.t, 24);
            std::memcpy(&vel[3 * (size_t)i], map.frames[i].v, 24);
        }
        std::vector<sadvio_imu_factor> fs;
        for (const ImuPair& p : map.imu_pairs) {                                          // :485-500
            if (p.frame_i == p.frame_j || p.frame_i < 0 || p.frame_j < 0 || p.frame_i >= n || p.frame_j >= n) continue;
            if (!map.frames[p.frame_i].has_imu || !map.frames[p.frame_j].has_imu) continue;
            sadvio_imu_factor f = p.f; f.kf_i = p.frame_i; f.kf_j = p.frame_j;
            fs.push_back(f);
        }
        sadvio_viinit_problem pb{};
        pb.n_frames = n; pb.n_factors = (int)fs.size(); pb.T_f_w = T.data(); pb.vel = vel.data(); pb.factors = fs.data();
        pb.optim_scale = optim_scale ? 1 : 0; pb.optim_bias = 0; pb.sigma_dba = pb.sigma_dbg = 1.0;
        sadvio_solve_options o; sadvio_ba_default_options(&o);
        o.max_num_iterations = 50;                                                        // :519-527
        sadvio_viinit_result r{};
        const int rc = sadvio_ba_vi_init(_h, &pb, &o, &_sum, &r, dv.data());
        const double I3[9] = {1, 0, 0, 0, 1, 0, 0, 0, 1};
        if (R_w_i) std::memcpy(R_w_i, I3, sizeof(I3));
        if (rc != SADVIO_OK) { _err = sadvio_ba_last_error(_h); return 1.0; }
        if (R_w_i) std::memcpy(R_w_i, r.R_w_i, sizeof(r.R_w_i));
        const double s = r.scale;
        for (int i = 0; i < n; i++) {
            FrameState& f = map.frames[i];
            if (f.has_imu) for (int a = 0; a < 3; a++) f.v[a] += dv[3 * (size_t)i + a];   // :526-531
            double Rn[9];
            for (int a = 0; a < 3; a++)
                for (int b = 0; b < 3; b++) Rn[3 * a + b] = f.T_f_w.R[3 * a] * r.R_w_i[b] + f.T_f_w.R[3 * a + 1] * r.R_w_i[3 + b] + f.T_f_w.R[3 * a + 2] * r.R_w_i[6 + b];
            std::memcpy(f.T_f_w.R, Rn, sizeof(Rn));
            for (int a = 0; a < 3; a++) f.T_f_w.t[a] *= s;                                 // :541-548
            if (f.has_prior) { f.T_prior = f.T_f_w; for (double& x : f.inf_prior) x = 100.0; }   // :550-552
        }
        for (LandmarkState& L : map.landmarks) {                                          // :555-562
            if (L.outlier) continue;
            double q[3];
            for (int a = 0; a < 3; a++) q[a] = s * (r.R_w_i[a] * L.p[0] + r.R_w_i[3 + a] * L.p[1] + r.R_w_i[6 + a] * L.p[2]);
            std::memcpy(L.p, q, sizeof(q));
        }
        return s;
    }

    // AngularAdjustmentCERESAnalytic::landmarkOptimizationNoFov (AngularAdjustmentCERESAnalytic.cpp:741-907): the metric scale
    // of T_cam0_cam0p from the landmarks f and fp share (nofov_flatten), Huber(sqrt(1.345)), 20 iterations (:857-868). Returns
    // false and changes nothing when the solution is not usable or lambda is outside [0.5, 1.5] (:870-871). Otherwise
    // T_cam0_cam0p.t *= lambda, fp's T_f_w = (f's T_w_f * T_f_s0 * T_cam0_cam0p * T_s0_f)^-1 (:874-877), and every landmark of the
    // problem is flagged outlier if its scale factor at the solution exceeds 2 / focal, else moved by its delta (:880-899).
    bool landmarkOptimizationNoFov(LocalMapSnapshot& map, int f, int fp, Pose& T_cam0_cam0p, double info_scale) {
        NoFovFlat F;
        if (!nofov_flatten(map, f, fp, T_cam0_cam0p, info_scale, F)) { _err = "landmarkOptimizationNoFov: bad frame index"; return false; }
        sadvio_solve_options o; sadvio_ba_default_options(&o);
        o.huber_a = std::sqrt(1.345);                                                     // :753
        const int n = F.pb.n_lmk;
        std::vector<double> dl(3 * (size_t)std::max(n, 1)), gn(std::max(n, 1));
        std::vector<int32_t> inl(std::max(n, 1), 1);
        sadvio_nofov_result r{};
        r.lambda = 1.0;
        const int rc = sadvio_ba_nofov_scale(_h, &F.pb, &o, &_sum, &r, dl.data(), gn.data(), inl.data());
        // no landmark and a constant scale: nothing to solve, Ceres returns the start point (lambda = 1)
        if (rc == SADVIO_E_INVALID_ARG && n == 0) r.lambda = 1.0;
        else if (rc != SADVIO_OK) { _err = sadvio_ba_last_error(_h); return false; }
        for (double& x : T_cam0_cam0p.t) x *= r.lambda;                                   // :874
        const Pose& Ts0 = map.frames[f].cameras[0].T_s_f;
        const Pose T_f0_f0p = pose_mul(pose_mul(pose_inv(Ts0), T_cam0_cam0p), Ts0);      // :875-876
        map.frames[fp].T_f_w = pose_inv(pose_mul(pose_inv(map.frames[f].T_f_w), T_f0_f0p));   // :877
        for (int k = 0; k < n; k++) {                                                     // :880-899
            LandmarkState& L = map.landmarks[F.lmk_src[k]];
            if (!inl[k]) { L.outlier = true; continue; }
            for (int a = 0; a < 3; a++) L.p[a] += dl[3 * (size_t)k + a];
        }
        return true;
    }

    // BundleAdjustmentCERESAnalytic::marginalize (…Analytic.cpp:431-663) with Marginalization::preMarginalize
    // (marginalization.cpp:23-143) restated on the snapshot: frame0 (index into map.frames) is marginalised into a prior
    // on frame1's states (VIO) and on the landmarks frame0 shares with the rest of the window. Returns false when the
    // Schur complement is refused (fewer than 4 kept columns, marginalization.cpp:215-216): the prior is then cleared,
    // as the reference does (…Analytic.cpp:620-625). The prior is held by this object (like _marginalization_last)
    // and added to the next localMapBA / localMapVIOptimization whose snapshot still contains its variables (by id).
    bool marginalize(LocalMapSnapshot& map, int frame0, int frame1, bool enable_sparsif) {
        const int nkf = (int)map.frames.size();
        if (frame0 < 0 || frame0 >= nkf || frame1 < 0 || frame1 >= nkf || frame0 == frame1) { _err = "marginalize: bad frame index"; return false; }
        Flat F;
        flatten(map, 0, map.frames[frame0].has_imu || map.frames[frame1].has_imu, false, false, F);
        // landmark selection (marginalization.cpp:50-88)
        std::vector<int32_t> keep, marg;
        std::vector<int> flat_of(map.landmarks.size(), -1);
        for (size_t k = 0; k < F.lmk_src.size(); k++) flat_of[F.lmk_src[k]] = (int)k;
        for (size_t l = 0; l < map.landmarks.size(); l++) {
            LandmarkState& L = map.landmarks[l];
            if (L.outlier || !L.in_map || !L.initialized) continue;
            bool in_frame0 = false, lonely = true;
            int num_cam = 0;
            for (const Feature& ft : L.features) {
                if (ft.frame != frame0) lonely = false; else { num_cam++; in_frame0 = true; }
            }
            if (!in_frame0) continue;                       // only the landmarks of frame0 are visited (:51)
            if (num_cam != 2 && !L.has_prior) continue;     // no full 3D information and no prior: ignored (:72-75)
            if (!lonely) { L.has_prior = true; keep.push_back(flat_of[l]); }
            else marg.push_back(flat_of[l]);
        }
        // resurrected landmarks of the previous prior (:116-139)
        bool discard_prior = false;
        if (_prior.valid)
            for (size_t q = 0; q < _prior.lmk_id.size() && !discard_prior; q++) {
                int idx = -1;
                for (size_t l = 0; l < map.landmarks.size(); l++) if (map.landmarks[l].id == _prior.lmk_id[q]) idx = (int)l;
                if (idx < 0 || flat_of[idx] < 0) { if (idx >= 0 && map.landmarks[idx].outlier) discard_prior = true; continue; }
                bool known = false;
                for (int32_t k : keep) known |= k == flat_of[idx];
                for (int32_t k : marg) known |= k == flat_of[idx];
                if (!known) keep.push_back(flat_of[idx]);
            }
        if (discard_prior) _prior = Prior();
        sadvio_marg_request rq{};
        rq.kf_marg = frame0;
        rq.marg_has_imu = map.frames[frame0].has_imu ? 1 : 0;
        rq.kf_keep = map.frames[frame1].has_imu ? frame1 : -1;                          // marginalization.cpp:99-104
        rq.n_marg = (int)marg.size(); rq.lmk_marg = marg.data();
        rq.n_keep = (int)keep.size(); rq.lmk_keep = keep.data();
        sadvio_imu_factor imu{};
        if (map.frames[frame0].has_imu && map.frames[frame1].has_imu)                  // …Analytic.cpp:449
            for (const ImuPair& p : map.imu_pairs)
                if (p.frame_i == frame0 && p.frame_j == frame1) { imu = p.f; rq.imu = &imu; }
        std::vector<sadvio_pose_prior> pri;
        // frame0's PosePriordx (…Analytic.cpp:605-617); the angular backend also folds in frame1's (Angular….cpp:682)
        for (const sadvio_pose_prior& p : F.priors) if (p.kf == frame0 || (_angular && p.kf == frame1)) pri.push_back(p);
        rq.n_prior = (int)pri.size(); rq.priors = pri.data();
        std::vector<int32_t> last_idx, last_col;
        // the previous prior is folded in whenever it kept landmarks (:573); its kept frame — VIO only — is frame0 now.
        // A VO prior (kf_col < 0) has no frame to match
        if (_prior.valid && !_prior.lmk_id.empty() && (_prior.kf_col < 0 || _prior.kf_id == map.frames[frame0].id)) {
            rq.last_n_full = SADVIO_PRIOR_RESIDENT;   // the prior never left the device (the handle holds it, AOptimizer.h:88-90)
            rq.last_kf = _prior.kf_col >= 0 ? frame0 : -1; rq.last_kf_col = std::max(_prior.kf_col, 0);
            for (size_t q = 0; q < _prior.lmk_id.size(); q++) {
                int fi = -1;
                for (size_t k = 0; k < F.lmk_id.size(); k++) if (F.lmk_id[k] == _prior.lmk_id[q]) fi = (int)k;
                last_idx.push_back(fi < 0 ? 0 : fi); last_col.push_back(fi < 0 ? -1 : _prior.lmk_col[q]);
            }
            rq.last_n_keep = (int)last_idx.size(); rq.last_lmk_index = last_idx.data(); rq.last_lmk_col = last_col.data();
        }
        rq.eig_cut_mode = _eig_cut_mode; rq.prior_form = _prior_form;
        std::vector<int32_t> lcol(std::max<size_t>(keep.size(), 1));
        sadvio_marg_result res{};
        if (F.non_pinhole_pixel) {   // the reference's own pixel factor has no Jacobian for these models (fisheye.cpp:352-405)
            _err = "pixel factor with a non-pinhole camera: use the angular backend (HipOptimizer(device, true))";
            return false;
        }
        int rc = upload(F);
        if (rc == SADVIO_OK) rc = sadvio_ba_marginalize(_h, 0, &rq, &res, lcol.data(), nullptr, nullptr);   // J, r0 stay on the device
        _prior = Prior(); _sparse.clear(); _sparse_lmk_id.clear();
        if (rc != SADVIO_OK) {
            if (rc != SADVIO_E_REFUSED) { _err = sadvio_ba_last_error(_h); sadvio_ba_set_prior(_h, 0, 0, 0, nullptr, nullptr); }   // no stale prior behind a failed call
            return false;
        }
        _prior.valid = res.n_full > 0; _prior.n_full = res.n_full; _prior.n = res.n;
        _prior.kf_id = rq.kf_keep >= 0 ? map.frames[frame1].id : -1; _prior.kf_col = res.kf_col;
        for (size_t k = 0; k < keep.size(); k++) { _prior.lmk_id.push_back(F.lmk_id[keep[k]]); _prior.lmk_col.push_back(lcol[k]); }
        if (enable_sparsif && keep.size() > 1) {
            std::vector<sadvio_sparse_prior> out(keep.size() + 1);
            int32_t n_out = 0;
            rc = sadvio_ba_sparsify(_h, 0, rq.kf_keep >= 0, 0, 0, nullptr /* the handle's prior */, rq.kf_keep, std::max(res.kf_col, 0),
                                    (int)keep.size(), keep.data(), lcol.data(), &n_out, out.data());
            if (rc == SADVIO_OK) {
                _sparse.assign(out.begin(), out.begin() + n_out);
                _sparse_kf_id = rq.kf_keep >= 0 ? map.frames[frame1].id : -1;
                for (const sadvio_sparse_prior& s : _sparse) { _sparse_lmk_id.push_back(s.lmk0 >= 0 ? F.lmk_id[s.lmk0] : -1); _sparse_lmk_id.push_back(s.lmk1 >= 0 ? F.lmk_id[s.lmk1] : -1); }
            }
        }
        return true;
    }
    // BundleAdjustmentCERESAnalytic::marginalizeRelative (…Analytic.cpp:665-809): the 6 x 6 information of the relative pose
    // T_frame0_frame1 recovered from the landmarks both frames observe (Schur complement on the two poses, then the NFR
    // covariance recovery through the Relative6DPose Jacobian). Returns false — and leaves a zero matrix, as the reference
    // returns Zero(12, 12) — when the Schur complement is refused. inf36 row-major; Ak144 (optional) = _marginalization->_Ak.
    bool marginalizeRelative(LocalMapSnapshot& map, int frame0, int frame1, double* inf36, double* Ak144 = nullptr) {
        const int nkf = (int)map.frames.size();
        for (int i = 0; i < 36; i++) inf36[i] = 0.0;
        if (frame0 < 0 || frame0 >= nkf || frame1 < 0 || frame1 >= nkf || frame0 == frame1) { _err = "marginalizeRelative: bad frame index"; return false; }
        Flat F;
        flatten(map, 0, false, false, false, F);
        if (F.non_pinhole_pixel) { _err = "pixel factor with a non-pinhole camera: use the angular backend"; return false; }
        double Ak[144];
        int rc = upload(F, false);
        if (rc == SADVIO_OK) rc = sadvio_ba_marginalize_relative(_h, 0, frame0, frame1, _rel_eig_cut_mode, inf36, Ak);
        if (rc != SADVIO_OK) { _err = sadvio_ba_last_error(_h); for (int i = 0; i < 36; i++) inf36[i] = 0.0; return false; }
        if (Ak144) std::memcpy(Ak144, Ak, sizeof(Ak));
        return true;
    }
    // marginalizeRelative for every (frame0, frame1) of `frames` (indices into map.frames) in one call
    // (sadvio_ba_marginalize_relative_batch): the snapshot is flattened and uploaded once, one kernel launch serves all pairs.
    // inf36: [n][36] row-major, T_a_b (optional): [n][12] = T_frame0_frame1 (R row-major 9 | t 3), the T_prior of the pair's
    // Relative6DPose factor, ok (optional): [n] 1 / 0. A refused pair (no shared landmark, singular covariance) has ok = 0 and
    // zeros, as marginalizeRelative leaves a zero matrix. Returns false, with every output zero, when the call itself fails (a
    // bad frame index, frame0 == frame1, a non-pinhole pixel camera).
    bool marginalizeRelativeBatch(LocalMapSnapshot& map, const std::vector<std::pair<int, int>>& frames, std::vector<double>* inf36,
                                  std::vector<double>* T_a_b = nullptr, std::vector<int>* ok = nullptr) {
        const size_t n = frames.size();
        const int nkf = (int)map.frames.size();
        std::vector<double> inf_local;
        std::vector<double>& inf = inf36 ? *inf36 : inf_local;
        inf.assign(36 * n, 0.0);
        if (T_a_b) T_a_b->assign(12 * n, 0.0);
        if (ok) ok->assign(n, 0);
        if (n == 0) return true;
        std::vector<int32_t> a(n), b(n), st(n, 0);
        for (size_t i = 0; i < n; i++) {
            a[i] = frames[i].first; b[i] = frames[i].second;
            if (a[i] < 0 || a[i] >= nkf || b[i] < 0 || b[i] >= nkf || a[i] == b[i]) { _err = "marginalizeRelativeBatch: bad frame index"; return false; }
        }
        Flat F;
        flatten(map, 0, false, false, false, F);
        if (F.non_pinhole_pixel) { _err = "pixel factor with a non-pinhole camera: use the angular backend"; return false; }
        int rc = upload(F, false);
        if (rc == SADVIO_OK)
            rc = sadvio_ba_marginalize_relative_batch(_h, 0, (int32_t)n, a.data(), b.data(), _rel_eig_cut_mode, inf.data(), nullptr,
                                                      T_a_b ? T_a_b->data() : nullptr, nullptr, st.data());
        if (rc != SADVIO_OK) {
            _err = sadvio_ba_last_error(_h);
            inf.assign(36 * n, 0.0);
            if (T_a_b) T_a_b->assign(12 * n, 0.0);
            return false;
        }
        if (ok) for (size_t i = 0; i < n; i++) (*ok)[i] = st[i] == SADVIO_OK ? 1 : 0;
        return true;
    }

    // Marginal covariances of the last window solve of this optimizer (sadvio_ba_covariance), addressed by the snapshot's ids:
    // frame_ids -> kf_cov [n][d][d] (d = block_dim(): 6, or 15 = pose6 | v | ba | bg after a VIO solve), frame_pairs -> pair_cov
    // [n][d][d] (rows first, columns second), landmark_ids -> lmk_cov [n][9]; any output may be null. Blocks are over the library's
    // delta coordinates at the written-back state; pose_covariance_ros maps a key-frame's leading 6 x 6 block to T_w_f. A frame that
    // was constant in the solve or a landmark the solve held constant gives zeros; a landmark with a rank-deficient H_ll gives NaN and
    // is counted in n_lmk_singular. Returns false (last_error says why) for an id the last window did not hold, when no window solve
    // precedes the call (a chi2-gated solve that re-uploaded its window counts as none), and when the gauge is not fixed.
    bool covariance(const std::vector<int64_t>& frame_ids, const std::vector<std::pair<int64_t, int64_t>>& frame_pairs,
                    const std::vector<int64_t>& landmark_ids, std::vector<double>* kf_cov, std::vector<double>* pair_cov,
                    std::vector<double>* lmk_cov, int* n_lmk_singular = nullptr) {
        auto find = [](const std::vector<int64_t>& ids, int64_t id) {
            for (size_t i = 0; i < ids.size(); i++) if (ids[i] == id) return (int32_t)i;
            return (int32_t)-1;
        };
        std::vector<int32_t> kf, pa, pb, lm;
        for (int64_t id : frame_ids) kf.push_back(find(_cov_kf_id, id));
        for (const auto& pr : frame_pairs) { pa.push_back(find(_cov_kf_id, pr.first)); pb.push_back(find(_cov_kf_id, pr.second)); }
        for (int64_t id : landmark_ids) lm.push_back(find(_cov_lmk_id, id));
        for (const std::vector<int32_t>* v : {&kf, &pa, &pb, &lm})
            for (int32_t i : *v) if (i < 0) { _err = "covariance: an id is not part of the last solved window"; return false; }
        const size_t dd = (size_t)_cov_dim * _cov_dim;
        std::vector<double> kc(dd * kf.size()), pc(dd * pa.size()), lc(9 * lm.size());
        sadvio_cov_request rq{};
        rq.n_kf = (int32_t)kf.size(); rq.kf = kf.data();
        rq.n_pair = (int32_t)pa.size(); rq.pair_a = pa.data(); rq.pair_b = pb.data();
        rq.n_lmk = (int32_t)lm.size(); rq.lmk = lm.data();
        int32_t ns = 0;
        const int rc = sadvio_ba_covariance(_h, 0, &rq, kf_cov && !kf.empty() ? kc.data() : nullptr, pair_cov && !pa.empty() ? pc.data() : nullptr,
                                            lmk_cov && !lm.empty() ? lc.data() : nullptr, &ns);
        if (rc != SADVIO_OK) { _err = sadvio_ba_last_error(_h); return false; }
        if (kf_cov) kf_cov->swap(kc);
        if (pair_cov) pair_cov->swap(pc);
        if (lmk_cov) lmk_cov->swap(lc);
        if (n_lmk_singular) *n_lmk_singular = ns;
        return true;
    }
    int block_dim() const { return _cov_dim; }   // 6 or 15: of the last window solve

    // Cross covariances Sigma(frame, landmark) of the last window solve and the innovation gate of candidate observations
    // (sadvio_ba_covariance_cross), addressed by the snapshot's ids as covariance() is: candidate i is (frame_ids[i], landmark_ids[i]).
    // cross_cov [n][d][3] (d = block_dim()). With cams (camera of each candidate, the rig's order) and meas ([n][2] pixel uv, or
    // [n][3] unit bearings for an angular solve): innov_cov [n][4], the 2 x 2 covariance of the whitened residual, and maha2 [n]
    // (innovation_gate turns it into a decision); without cams both must be null. A camera is named as Feature::camera names it: its
    // index among the cameras of the candidate's frame. status [n]: SADVIO_CROSS_*. Any output may be null. Returns false (last_error
    // says why) as covariance() does.
    bool covarianceCross(const std::vector<int64_t>& frame_ids, const std::vector<int64_t>& landmark_ids, const std::vector<int32_t>* cams,
                         const std::vector<double>* meas, std::vector<double>* cross_cov, std::vector<double>* innov_cov,
                         std::vector<double>* maha2, std::vector<int32_t>* status = nullptr) {
        auto find = [](const std::vector<int64_t>& ids, int64_t id) {
            for (size_t i = 0; i < ids.size(); i++) if (ids[i] == id) return (int32_t)i;
            return (int32_t)-1;
        };
        const size_t n = frame_ids.size();
        if (landmark_ids.size() != n || (cams && cams->size() != n) || ((cams == nullptr) != (meas == nullptr))) {
            _err = "covarianceCross: the candidate arrays differ in length";
            return false;
        }
        std::vector<int32_t> kf, lm;
        for (int64_t id : frame_ids) kf.push_back(find(_cov_kf_id, id));
        for (int64_t id : landmark_ids) lm.push_back(find(_cov_lmk_id, id));
        for (const std::vector<int32_t>* v : {&kf, &lm})
            for (int32_t i : *v) if (i < 0) { _err = "covarianceCross: an id is not part of the last solved window"; return false; }
        std::vector<double> xc(3 * (size_t)_cov_dim * n), pc(4 * n), m2(n);
        std::vector<int32_t> st(n);
        sadvio_cov_cross_request rq{};
        rq.n = (int32_t)n; rq.kf = kf.data(); rq.lmk = lm.data();
        std::vector<int32_t> wc;   // window camera = first camera of the frame + the camera's index in the frame
        if (cams) {
            for (size_t i = 0; i < n; i++) {
                const int32_t last = (size_t)kf[i] + 1 < _cov_cam_base.size() ? _cov_cam_base[(size_t)kf[i] + 1] : _cov_n_cam;
                if ((size_t)kf[i] >= _cov_cam_base.size() || (*cams)[i] < 0 || _cov_cam_base[kf[i]] + (*cams)[i] >= last) {
                    _err = "covarianceCross: camera index out of range";
                    return false;
                }
                wc.push_back(_cov_cam_base[kf[i]] + (*cams)[i]);
            }
        }
        rq.cam = cams ? wc.data() : nullptr; rq.meas = meas ? meas->data() : nullptr;
        const int rc = sadvio_ba_covariance_cross(_h, 0, &rq, cross_cov && n ? xc.data() : nullptr, innov_cov && n ? pc.data() : nullptr,
                                                  maha2 && n ? m2.data() : nullptr, status && n ? st.data() : nullptr);
        if (rc != SADVIO_OK) { _err = sadvio_ba_last_error(_h); return false; }
        if (cross_cov) cross_cov->swap(xc);
        if (innov_cov) innov_cov->swap(pc);
        if (maha2) maha2->swap(m2);
        if (status) status->swap(st);
        return true;
    }

    bool has_prior() const { return _prior.valid; }
    int prior_rows() const { return _prior.n_full; }
    int prior_cols() const { return _prior.n; }
    // n_full x n row-major, read back from the device on request (sadvio_ba_get_prior): the solve path never needs it on the host
    // Route counters of this optimizer's Cholesky-form marginalisations (sadvio_ba_marg_stats): {calls, unpivoted, fell_back}
    std::array<int32_t, 3> marg_stats() const {
        std::array<int32_t, 3> v{0, 0, 0};
        (void)sadvio_ba_marg_stats(_h, &v[0], &v[1], &v[2]);
        return v;
    }
    // Read-backs over PCIe (not for per-frame use); the buffers are sized from what the HANDLE reports, not from this object's copy
    // of the shape, so a divergence between the two cannot overflow them.
    std::vector<double> prior_J() const {
        sadvio_prior_info pi{};
        if (!_prior.valid || sadvio_ba_get_prior(_h, &pi, nullptr, nullptr) != SADVIO_OK || !pi.valid) return {};
        std::vector<double> J((size_t)pi.n_full * (size_t)pi.n);
        if (sadvio_ba_get_prior(_h, nullptr, J.data(), nullptr) != SADVIO_OK) J.clear();
        return J;
    }
    std::vector<double> prior_r0() const {
        sadvio_prior_info pi{};
        if (!_prior.valid || sadvio_ba_get_prior(_h, &pi, nullptr, nullptr) != SADVIO_OK || !pi.valid) return {};
        std::vector<double> r((size_t)pi.n_full);
        if (sadvio_ba_get_prior(_h, nullptr, nullptr, r.data()) != SADVIO_OK) r.clear();
        return r;
    }
    // Eigenvalue cut of marginalize / marginalizeRelative (SADVIO_EIG_CUT_*; default: the reference's absolute 1e-12,
    // marginalization.hpp:58) and form of the stored prior (SADVIO_PRIOR_FORM_*; default: the rank-revealing Cholesky factor —
    // same MarginalizationFactor cost / gradient / Gauss-Newton matrix as the reference's Lambda^1/2 U^T, 5 x faster to form;
    // SADVIO_PRIOR_FORM_EIGEN reproduces the reference's rows).
    void set_eig_cut_mode(int mode) { _eig_cut_mode = mode; }
    // marginalizeRelative keeps the noise floor by default: Ak of two poses has an EXACT 6-dimensional gauge null space whose
    // eigenvalues compute to +-1e-7 .. 1e-6; the reference's absolute 1e-12 inverts the positive ones (1 / lambda ~ 1e6) and the
    // recovered 6 x 6 'information' is then rounding noise (measured through this layer: trace 6.9e6, min diagonal -4.9e5) —
    // the reference's own function has no caller. SADVIO_EIG_CUT_REFERENCE reproduces it on request.
    void set_relative_eig_cut_mode(int mode) { _rel_eig_cut_mode = mode; }
    void set_prior_form(int form) { _prior_form = form; }
    const std::vector<int64_t>& prior_landmark_ids() const { return _prior.lmk_id; }
    const std::vector<int32_t>& prior_landmark_cols() const { return _prior.lmk_col; }
    size_t sparse_factor_count() const { return _sparse.size(); }
    // features the last flattened window left out because their camera index was outside the frame's sensor list (also warned on stderr)
    int skipped_bad_camera_features() const { return _skipped_bad_camera; }

    const sadvio_solve_summary& summary() const { return _sum; }
    const std::string& last_error() const { return _err; }
    // every window handed to the backend is also written to <dir>/window_NNNNNN.sadvio (include/sadvio_io.hpp)
    void set_dump_dir(const std::string& dir) { _dump_dir = dir; _dump_count = 0; }

    // ALandmark::sanityCheck of maps with non-pinhole cameras: off (default) = the host loop host_chi2_gate; on = the device
    // gate sadvio_ba_landmark_chi2_models, with the models of CameraModel::intrinsics() and the features' own pixels
    void set_device_model_gate(bool on) { _device_model_gate = on; }

  private:
    struct Flat {   // the flattened window + the vectors it points into
        sadvio_flat_window w{};
        std::vector<int64_t> kf_id, lmk_id;
        std::vector<double> kf_T, kf_v, kf_ba, kf_bg, cam_K, cam_T, cam_sigma, lmk_p, meas;
        std::vector<uint8_t> kf_const, lc;
        std::vector<int> cam_base, lmk_src;
        std::vector<double> cam_wh;       // image size per flat camera (sanityCheck)
        std::vector<sadvio_camera_model> cam_model;   // the model per flat camera, the feature's pixel per observation:
        std::vector<double> obs_uv;                   // what sadvio_ba_landmark_chi2_models takes (sanityCheck on non-pinhole rigs)
        int n_non_kf_obs = 0;             // features skipped because their frame is not a key-frame
        int n_bad_camera = 0;             // features skipped because their camera index is not one of the frame's sensors
        bool any_non_pinhole = false, non_pinhole_pixel = false;
        std::vector<int32_t> ptr, obs_kf, obs_cam;
        std::vector<sadvio_pose_prior> priors;
        std::vector<sadvio_imu_factor> imus;
        // linexd landmarks (…Analytic.cpp:270-310)
        std::vector<int> line_src;
        std::vector<int64_t> line_id;
        std::vector<double> line_T, line_model, line_meas;
        std::vector<int32_t> line_ptr, line_obs_kf, line_obs_cam;
        sadvio_line_set lines{};
    };
    struct Prior {  // the dense prior kept between marginalize() and the next window solves, variables named by id
        bool valid = false;
        int n_full = 0, n = 0, kf_col = -1;
        int64_t kf_id = -1;
        std::vector<int64_t> lmk_id;   // J, r0 themselves live in the backend handle (device resident)
        std::vector<int32_t> lmk_col;
    };

    // inclusion rules of addResidualsLocalMap (BundleAdjustmentCERESAnalytic.cpp:197-314)
    void flatten(const LocalMapSnapshot& map, size_t fixed, bool vio, bool all_const, bool lmk_const, Flat& F, bool kf_only = true) const {
        const int nkf = (int)map.frames.size();
        F.kf_id.resize(nkf); F.kf_T.resize(12 * (size_t)nkf); F.kf_v.resize(3 * (size_t)nkf); F.kf_ba.resize(3 * (size_t)nkf);
        F.kf_bg.resize(3 * (size_t)nkf); F.kf_const.resize(nkf); F.cam_base.resize(nkf); F.ptr.assign(1, 0);
        for (int i = 0; i < nkf; i++) {
            const FrameState& f = map.frames[i];
            F.kf_id[i] = f.id;
            std::memcpy(&F.kf_T[12 * (size_t)i], f.T_f_w.R, 72); std::memcpy(&F.kf_T[12 * (size_t)i + 9], f.T_f_w.t, 24);
            std::memcpy(&F.kf_v[3 * (size_t)i], f.v, 24); std::memcpy(&F.kf_ba[3 * (size_t)i], f.ba, 24); std::memcpy(&F.kf_bg[3 * (size_t)i], f.bg, 24);
            F.kf_const[i] = all_const || (i > nkf - (int)fixed - 1);                     // …Analytic.cpp:219
            if (f.has_prior) {                                                           // :224-228
                sadvio_pose_prior p{};
                p.kf = i; std::memcpy(p.T_prior, f.T_prior.R, 72); std::memcpy(p.T_prior + 9, f.T_prior.t, 24);
                std::memcpy(p.inf_diag, f.inf_prior, 48);
                F.priors.push_back(p);
            }
            F.cam_base[i] = (int)F.cam_sigma.size();
            for (const CameraModel& c : f.cameras) {
                const double K[4] = {c.fx, c.fy, c.cx, c.cy};
                F.cam_K.insert(F.cam_K.end(), K, K + 4);
                F.cam_T.insert(F.cam_T.end(), c.T_s_f.R, c.T_s_f.R + 9); F.cam_T.insert(F.cam_T.end(), c.T_s_f.t, c.T_s_f.t + 3);
                F.cam_sigma.push_back(_angular ? 1.5 / (0.5 * (c.fx + c.fy)) : 1.0);    // …Analytic.h:46 / Angular….cpp:283
                F.cam_wh.push_back(c.width > 0 ? c.width : 2.0 * c.cx); F.cam_wh.push_back(c.height > 0 ? c.height : 2.0 * c.cy);
                const CameraIntrinsics ci = c.intrinsics();
                static_assert((int)CameraKind::Pinhole == SADVIO_CAM_PINHOLE && (int)CameraKind::FisheyeEquidistant == SADVIO_CAM_FISHEYE_EQUIDISTANT &&
                              (int)CameraKind::FisheyeEquisolid == SADVIO_CAM_FISHEYE_EQUISOLID && (int)CameraKind::FisheyeStereographic == SADVIO_CAM_FISHEYE_STEREOGRAPHIC &&
                              (int)CameraKind::Omni == SADVIO_CAM_OMNI && (int)CameraKind::DoubleSphere == SADVIO_CAM_DOUBLE_SPHERE, "CameraKind follows SADVIO_CAM_*");
                sadvio_camera_model cm{};
                cm.kind = (int32_t)ci.kind; cm.distortion = ci.distortion ? 1 : 0; cm.width = ci.width; cm.height = ci.height;
                cm.rmax = ci.rmax; cm.xi = ci.xi; cm.alpha = ci.alpha;
                for (int a = 0; a < 4; a++) cm.D[a] = ci.D[a];
                F.cam_model.push_back(cm);
            }
        }
        for (int l = 0; l < (int)map.landmarks.size(); l++) {
            const LandmarkState& L = map.landmarks[l];
            if (!L.initialized || L.outlier) continue;                                   // :239
            F.lmk_src.push_back(l); F.lmk_id.push_back(L.id); F.lc.push_back(lmk_const ? 1 : 0);
            F.lmk_p.insert(F.lmk_p.end(), L.p, L.p + 3);
            for (const Feature& ft : L.features) {
                if (ft.frame < 0 || ft.frame >= nkf) continue;                           // :256-258 (frame not in the window)
                if (kf_only && !map.frames[ft.frame].is_keyframe) { F.n_non_kf_obs++; continue; }   // :131, :256
                if (ft.camera < 0 || ft.camera >= (int)map.frames[ft.frame].cameras.size()) { F.n_bad_camera++; continue; }   // a feature of a sensor the frame does not carry
                const CameraModel& c = map.frames[ft.frame].cameras[ft.camera];
                F.obs_kf.push_back(ft.frame); F.obs_cam.push_back(F.cam_base[ft.frame] + ft.camera);
                F.obs_uv.push_back(ft.u); F.obs_uv.push_back(ft.v);
                if (_angular) {                                                          // getRayCamera of the feature's camera model
                    double b[3] = {0.0, 0.0, 1.0};
                    ray_camera(c.intrinsics(), ft.u, ft.v, b);
                    F.meas.insert(F.meas.end(), {b[0], b[1], b[2]});
                } else {
                    if (c.kind != CameraKind::Pinhole) F.non_pinhole_pixel = true;           // no analytic pixel factor exists for it
                    F.meas.insert(F.meas.end(), {ft.u, ft.v});
                }
                if (c.kind != CameraKind::Pinhole) F.any_non_pinhole = true;
            }
            F.ptr.push_back((int32_t)F.obs_kf.size());
        }
        F.line_ptr.assign(1, 0);
        for (int l = 0; l < (int)map.lines.size(); l++) {                                // …Analytic.cpp:270-310
            const LineLandmarkState& L = map.lines[l];
            if (!L.initialized || L.outlier) continue;
            F.line_src.push_back(l); F.line_id.push_back(L.id);
            F.line_T.insert(F.line_T.end(), L.T_w_l.R, L.T_w_l.R + 9); F.line_T.insert(F.line_T.end(), L.T_w_l.t, L.T_w_l.t + 3);
            F.line_model.insert(F.line_model.end(), L.model, L.model + 6);
            for (const LineFeature& ft : L.features) {
                if (ft.frame < 0 || ft.frame >= nkf || !map.frames[ft.frame].is_keyframe) continue;   // :296-299
                if (ft.camera < 0 || ft.camera >= (int)map.frames[ft.frame].cameras.size()) { F.n_bad_camera++; continue; }
                const CameraModel& c = map.frames[ft.frame].cameras[ft.camera];
                F.line_obs_kf.push_back(ft.frame); F.line_obs_cam.push_back(F.cam_base[ft.frame] + ft.camera);
                if (_angular) {                                                          // feature->getBearingVectors()
                    double b0[3] = {0, 0, 1}, b1[3] = {0, 0, 1};
                    ray_camera(c.intrinsics(), ft.u0, ft.v0, b0); ray_camera(c.intrinsics(), ft.u1, ft.v1, b1);
                    F.line_meas.insert(F.line_meas.end(), {b0[0], b0[1], b0[2], b1[0], b1[1], b1[2]});
                } else {
                    if (c.kind != CameraKind::Pinhole) F.non_pinhole_pixel = true;
                    F.line_meas.insert(F.line_meas.end(), {ft.u0, ft.v0, ft.u1, ft.v1});
                }
            }
            F.line_ptr.push_back((int32_t)F.line_obs_kf.size());
        }
        F.lines.n_line = (int)F.line_src.size(); F.lines.n_obs = (int)F.line_obs_kf.size();
        F.lines.line_id = F.line_id.data(); F.lines.line_T_w_l = F.line_T.data(); F.lines.line_model = F.line_model.data();
        F.lines.line_const = nullptr; F.lines.line_obs_ptr = F.line_ptr.data();
        F.lines.obs_kf = F.line_obs_kf.data(); F.lines.obs_cam = F.line_obs_cam.data(); F.lines.obs_meas = F.line_meas.data();
        if (vio)
            for (const ImuPair& p : map.imu_pairs) {                                     // AOptimizer.cpp:69-72
                if (p.frame_i == p.frame_j || p.f.dt > 1.0) continue;
                sadvio_imu_factor f = p.f; f.kf_i = p.frame_i; f.kf_j = p.frame_j;
                F.imus.push_back(f);
            }
        // (a landmark may carry more than 64 observations: the library solves such long tracks beside its landmark tiles, sadvio_ba.h)
        sadvio_flat_window& w = F.w;
        w.n_kf = nkf; w.n_cam = (int)F.cam_sigma.size(); w.n_lmk = (int)F.lmk_src.size(); w.n_obs = (int)F.obs_kf.size();
        w.factor_type = _angular ? SADVIO_FACTOR_ANGULAR : SADVIO_FACTOR_PIXEL; w.has_imu = vio ? 1 : 0;
        w.kf_id = F.kf_id.data(); w.kf_T_f_w = F.kf_T.data(); w.kf_const = F.kf_const.data();
        w.kf_vel = F.kf_v.data(); w.kf_ba = F.kf_ba.data(); w.kf_bg = F.kf_bg.data();
        w.cam_K = F.cam_K.data(); w.cam_T_s_f = F.cam_T.data(); w.cam_sigma = F.cam_sigma.data();
        w.lmk_id = F.lmk_id.data(); w.lmk_p = F.lmk_p.data(); w.lmk_const = F.lc.data(); w.lmk_obs_ptr = F.ptr.data();
        w.obs_kf = F.obs_kf.data(); w.obs_cam = F.obs_cam.data(); w.obs_meas = F.meas.data();
    }

    // with_pose_priors: PosePriordx blocks are only added by addResidualsLocalMap (…Analytic.cpp:224-228) and marginalize
    // (:605-617); addSingleFrameResiduals / addLandmarkResiduals (:5-50, 102-150) add none
    int upload(const Flat& F, bool with_pose_priors = true, const Flat* prior_of = nullptr) {
        // a feature whose camera index is not one of its frame's sensors cannot be evaluated: it is skipped (the reference would
        // throw from .at()), and the count is REPORTED — a corrupted map must not solve silently with fewer observations
        _skipped_bad_camera = F.n_bad_camera;
        if (F.n_bad_camera) std::fprintf(stderr, "[sadvio] warning: %d feature(s) skipped: camera index outside the frame's sensor list\n", F.n_bad_camera);
        // one layout build for the window and all its factor lists (sadvio_ba_begin_update .. commit_update)
        int rc = sadvio_ba_begin_update(_h);
        if (rc == SADVIO_OK) rc = sadvio_ba_set_windows(_h, 1, &F.w);
        if (rc == SADVIO_OK && with_pose_priors) rc = sadvio_ba_set_pose_priors(_h, 0, (int)F.priors.size(), F.priors.data());
        if (rc == SADVIO_OK && !F.imus.empty()) rc = sadvio_ba_set_imu_factors(_h, 0, (int)F.imus.size(), F.imus.data());
        if (rc == SADVIO_OK && prior_of) rc = add_marginalization_prior(*prior_of);
        const int rc2 = sadvio_ba_commit_update(_h);
        return rc != SADVIO_OK ? rc : rc2;
    }

    // addMarginalizationResiduals (…Analytic.cpp:316-426): the stored prior on the variables still in the window
    int add_marginalization_prior(const Flat& F) {
        if (!_sparse.empty()) {
            std::vector<sadvio_sparse_prior> fs;
            for (size_t k = 0; k < _sparse.size(); k++) {
                sadvio_sparse_prior s = _sparse[k];
                auto find_l = [&](int64_t id) { for (size_t q = 0; q < F.lmk_id.size(); q++) if (F.lmk_id[q] == id) return (int)q; return -1; };
                auto find_k = [&](int64_t id) { for (size_t q = 0; q < F.kf_id.size(); q++) if (F.kf_id[q] == id) return (int)q; return -1; };
                if (s.kf >= 0) { s.kf = find_k(_sparse_kf_id); if (s.kf < 0) continue; }
                if (s.lmk0 >= 0) { s.lmk0 = find_l(_sparse_lmk_id[2 * k]); if (s.lmk0 < 0) continue; }
                if (s.lmk1 >= 0) { s.lmk1 = find_l(_sparse_lmk_id[2 * k + 1]); if (s.lmk1 < 0) continue; }
                fs.push_back(s);
            }
            return fs.empty() ? SADVIO_OK : sadvio_ba_set_sparse_priors(_h, 0, (int)fs.size(), fs.data());
        }
        if (!_prior.valid) return SADVIO_OK;
        int kf = -1;
        if (_prior.kf_col >= 0) {
            for (size_t q = 0; q < F.kf_id.size(); q++) if (F.kf_id[q] == _prior.kf_id) kf = (int)q;
            if (kf < 0) return SADVIO_OK;   // the kept frame left the window: nothing to attach the prior to
        }
        std::vector<int32_t> idx, col;
        for (size_t q = 0; q < _prior.lmk_id.size(); q++) {
            int fi = -1;
            for (size_t k = 0; k < F.lmk_id.size(); k++) if (F.lmk_id[k] == _prior.lmk_id[q]) fi = (int)k;
            idx.push_back(fi < 0 ? 0 : fi); col.push_back(fi < 0 ? -1 : _prior.lmk_col[q]);   // absent landmark: zero delta
        }
        return sadvio_ba_set_dense_prior(_h, 0, SADVIO_PRIOR_RESIDENT, 0, nullptr, nullptr, kf, std::max(_prior.kf_col, 0),
                                         (int)idx.size(), idx.data(), col.data());
    }

    // ALandmark::sanityCheck on the host for maps with non-pinhole cameras: every feature of the landmark (key-frame or
    // not) is projected with its own camera model (sadvio_cameras.hpp) at the landmark's CURRENT position
    void host_chi2_gate(const LocalMapSnapshot& map, const Flat& F, std::vector<int32_t>& inlier) const {
        for (size_t k = 0; k < F.lmk_src.size(); k++) {
            const LandmarkState& L = map.landmarks[F.lmk_src[k]];
            double sum = 0.0;
            int n = 0;
            for (const Feature& ft : L.features) {
                if (ft.frame < 0 || ft.frame >= (int)map.frames.size()) continue;
                const FrameState& fr = map.frames[ft.frame];
                if (ft.camera < 0 || ft.camera >= (int)fr.cameras.size()) continue;
                const CameraModel& c = fr.cameras[ft.camera];
                double pf[3], pc[3], u, v;
                for (int a = 0; a < 3; a++) pf[a] = fr.T_f_w.R[3 * a] * L.p[0] + fr.T_f_w.R[3 * a + 1] * L.p[1] + fr.T_f_w.R[3 * a + 2] * L.p[2] + fr.T_f_w.t[a];
                for (int a = 0; a < 3; a++) pc[a] = c.T_s_f.R[3 * a] * pf[0] + c.T_s_f.R[3 * a + 1] * pf[1] + c.T_s_f.R[3 * a + 2] * pf[2] + c.T_s_f.t[a];
                const bool ok = project_camera(c.intrinsics(), pc, u, v);
                sum += ok ? (u - ft.u) * (u - ft.u) + (v - ft.v) * (v - ft.v) : 1000.0;   // feature sigma = 1 px (AFeature2D.h:18)
                n++;
            }
            inlier[k] = (n >= 2 && !(sum / n > 2.0)) ? 1 : 0;
        }
    }

    bool solve(LocalMapSnapshot& map, size_t fixed, bool vio, const sadvio_solve_options& opt, bool all_const, bool lmk_const,
               bool chi2_gate = false) {
        const int nkf = (int)map.frames.size();
        Flat F;
        flatten(map, fixed, vio, all_const, lmk_const, F, !lmk_const);   // addSingleFrameResiduals has no key-frame test (:5-50)
        if (!_dump_dir.empty()) {   // replayable record of exactly what the backend is given (scripts/replay.py)
            char name[64];
            std::snprintf(name, sizeof(name), "/window_%06d.sadvio", _dump_count++);
            const std::string e = write_window(_dump_dir + name, F.w, (!all_const && !lmk_const) ? (int)F.priors.size() : 0, F.priors.data(), (int)F.imus.size(), F.imus.data());
            if (!e.empty()) _err = e;
        }
        if (F.non_pinhole_pixel) {   // the reference's own pixel factor has no Jacobian for these models (fisheye.cpp:352-405)
            _err = "pixel factor with a non-pinhole camera: use the angular backend (HipOptimizer(device, true))";
            return false;
        }
        const bool window_solve = !all_const && !lmk_const;
        int rc = upload(F, window_solve, window_solve ? &F : nullptr);   // the stored prior rides the same layout build
        const bool with_lines = window_solve && F.lines.n_line > 0;      // the line blocks are only built by addResidualsLocalMap
        if (rc == SADVIO_OK && with_lines) rc = sadvio_ba_set_lines(_h, 0, &F.lines);
        if (rc == SADVIO_OK) rc = sadvio_ba_solve(_h, &opt, &_sum);
        if (rc != SADVIO_OK && rc != SADVIO_E_NOT_USABLE) { _err = sadvio_ba_last_error(_h); return false; }   // state untouched
        if (rc == SADVIO_E_NOT_USABLE) return false;
        _cov_kf_id = F.kf_id; _cov_lmk_id = F.lmk_id; _cov_dim = vio ? 15 : 6;   // what covariance() addresses
        _cov_cam_base = F.cam_base; _cov_n_cam = (int)F.cam_sigma.size();           // ... and where a frame's cameras start in the window
        std::vector<double> dpose(6 * (size_t)nkf), dl(3 * (size_t)std::max(F.w.n_lmk, 1)), dv(3 * (size_t)nkf), dba(3 * (size_t)nkf), dbg(3 * (size_t)nkf);
        if (sadvio_ba_get_deltas(_h, 0, dpose.data(), dl.data(), dv.data(), dba.data(), dbg.data()) != SADVIO_OK) { _err = sadvio_ba_last_error(_h); return false; }
        for (int i = 0; i < nkf; i++) {                                                  // AOptimizer.cpp:329-332
            apply_pose_delta(map.frames[i].T_f_w, &dpose[6 * (size_t)i]);
            if (vio)                                                                     // :405-418
                for (int a = 0; a < 3; a++) {
                    map.frames[i].v[a] += dv[3 * (size_t)i + a]; map.frames[i].ba[a] += dba[3 * (size_t)i + a]; map.frames[i].bg[a] += dbg[3 * (size_t)i + a];
                }
        }
        // IMU::biasDeltaCorrection (IMU.cpp:104-108) of every pre-integration whose older frame got a bias update
        // (AOptimizer.cpp:421-434): localMapVIOptimization only — singleFrameVIOptimization does not do it (:262-296)
        if (vio && window_solve)
            for (ImuPair& p : map.imu_pairs) {
                if (p.frame_i < 0 || p.frame_i >= nkf || p.frame_j < 0 || p.frame_j >= nkf || !map.frames[p.frame_j].has_imu || !map.frames[p.frame_i].has_imu) continue;
                bias_delta_correction(p.f, &dba[3 * (size_t)p.frame_i], &dbg[3 * (size_t)p.frame_i]);
            }
        if (with_lines) {                                                                // AOptimizer.cpp:334-336: T_w_l <- T_w_l * (exp(w), t)
            std::vector<double> d6(6 * (size_t)F.lines.n_line);
            if (sadvio_ba_get_line_deltas(_h, 0, d6.data()) != SADVIO_OK) { _err = sadvio_ba_last_error(_h); return false; }
            for (size_t k = 0; k < F.line_src.size(); k++) apply_pose_delta(map.lines[F.line_src[k]].T_w_l, &d6[6 * k]);
        }
        std::vector<int32_t> inlier(F.lmk_src.size(), 1);
        if (chi2_gate && !F.lmk_src.empty()) {                                           // ALandmark.cpp:130-146
            const Flat* G = &F;
            Flat Fall;
            if (F.n_non_kf_obs) {   // sanityCheck walks ALL the features of the landmark, key-frame or not
                flatten(map, fixed, vio, all_const, lmk_const, Fall, false);
                if (sadvio_ba_set_windows(_h, 1, &Fall.w) != SADVIO_OK) { _err = sadvio_ba_last_error(_h); return false; }
                G = &Fall;
            }
            if (F.any_non_pinhole && _device_model_gate) {           // every feature through its own camera model, on the device
                if (sadvio_ba_landmark_chi2_models(_h, 0, nullptr, nullptr, G->cam_model.data(), G->obs_uv.data(), 1.0, nullptr, inlier.data(), nullptr) != SADVIO_OK) {
                    _err = sadvio_ba_last_error(_h); return false;
                }
            } else if (F.any_non_pinhole) host_chi2_gate(map, F, inlier);   // sadvio_ba_landmark_chi2 projects with K only
            else if (sadvio_ba_landmark_chi2(_h, 0, nullptr, nullptr, G->cam_wh.data(), 1.0, nullptr, inlier.data()) != SADVIO_OK) {
                _err = sadvio_ba_last_error(_h); return false;
            }
        }
        for (size_t k = 0; k < F.lmk_src.size(); k++) {                                  // :334-340
            LandmarkState& L = map.landmarks[F.lmk_src[k]];
            if (chi2_gate) L.outlier = !inlier[k];                                       // setOutlier / setInlier
            if (inlier[k]) for (int a = 0; a < 3; a++) L.p[a] += dl[3 * k + a];
        }
        return true;
    }

    std::string _dump_dir;
    int _dump_count = 0;
    int _skipped_bad_camera = 0;
    bool _device_model_gate = false;
    int _eig_cut_mode = SADVIO_EIG_CUT_REFERENCE, _rel_eig_cut_mode = SADVIO_EIG_CUT_NOISE_FLOOR, _prior_form = SADVIO_PRIOR_FORM_CHOLESKY;
    sadvio_ba_handle* _h = nullptr;
    sadvio_solve_summary _sum{};
    std::string _err;
    bool _angular;
    Prior _prior;
    std::vector<sadvio_sparse_prior> _sparse;   // the sparsified prior (indices of the window it was built on)
    std::vector<int64_t> _sparse_lmk_id;        // [2 k], [2 k + 1]: ids of lmk0 / lmk1 of factor k
    int64_t _sparse_kf_id = -1;
    std::vector<int64_t> _cov_kf_id, _cov_lmk_id;   // ids of the last solved window, in its order
    std::vector<int> _cov_cam_base;                  // first window camera of each of its frames
    int _cov_n_cam = 0;
    int _cov_dim = 6;
};

}  // namespace sadvio
