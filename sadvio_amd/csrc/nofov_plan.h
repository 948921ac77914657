// nofov_plan.h — the host side of sadvio_ba_nofov_scale (landmarkOptimizationNoFov, AngularAdjustmentCERESAnalytic.cpp:741-907) that
// needs no device: the argument checks, the decision whether the scale is held constant, and the constant tables of k_nofov. Plain
// C++17 without the HIP runtime or the handle (tests/cpp/test_nofov_plan.cpp); nofov_driver.h holds the launch.
#pragma once
#include <algorithm>
#include <cmath>
#include <cstring>

#include "../../include/sadvio_ba.h"

// the sizes nofov_kernels.h gives these tables and limits (nofov_driver.h asserts that they agree)
constexpr int NOFOV_PLAN_FTAB = 39, NOFOV_PLAN_CTAB = 15, NOFOV_PLAN_MAX_LMK = 65536, NOFOV_PLAN_MAX_OBS_PER_LMK = 16;

// fix_scale = -1, :769-772: geometry::log_so3 (geometry.h:149-166) of the rotation, norm of the translation
inline int nofov_reference_fix_scale(const double* Tm) {
    double c = (Tm[0] + Tm[4] + Tm[8]) / 2.0 - 0.5;
    c = std::min(std::max(c, -1.0), 1.0);
    const double ang = std::acos(c);
    const double d[3] = {Tm[7] - Tm[5], Tm[2] - Tm[6], Tm[3] - Tm[1]};
    const double f = (std::fabs(std::sin(ang)) < 1e-9 || ang < 1e-9) ? 0.5 : ang / (2.0 * std::sin(ang));
    const double rot = f * std::sqrt(d[0] * d[0] + d[1] * d[1] + d[2] * d[2]);
    const double tn = std::sqrt(Tm[9] * Tm[9] + Tm[10] * Tm[10] + Tm[11] * Tm[11]);
    return (rot < 0.05 || tn < 0.01) ? 1 : 0;
}

// Why the problem is refused (SADVIO_E_INVALID_ARG with this text), or null; `fixed`: whether lambda is held constant
inline const char* nofov_check(const sadvio_nofov_problem* pb, const sadvio_solve_options* opts, int& fixed) {
    if (!pb || !opts || pb->n_lmk < 0 || pb->n_obs < 0 || pb->n_frames < 1 || pb->n_cam < 1 || !pb->frame_T_f_w || !pb->cam_T_s_f ||
        !pb->T_cam0_cam0p || pb->cam0 < 0 || pb->cam0 >= pb->n_cam || pb->fix_scale < -1 || pb->fix_scale > 1 ||
        (pb->n_lmk > 0 && (!pb->lmk_p || !pb->scale_bearing || !pb->scale_cam || !pb->lmk_obs_ptr)) ||
        (pb->n_obs > 0 && (!pb->obs_frame || !pb->obs_cam || !pb->obs_bearing || !pb->lmk_obs_ptr)))
        return "nofov_scale: bad argument";
    const int n = pb->n_lmk, no = pb->n_obs, nfr = pb->n_frames, nc = pb->n_cam;
    if (n > NOFOV_PLAN_MAX_LMK) return "nofov_scale: more than 65536 landmarks";
    if (n > 0) {
        if (pb->lmk_obs_ptr[0] != 0 || pb->lmk_obs_ptr[n] != no) return "nofov_scale: lmk_obs_ptr does not span n_obs";
        for (int l = 0; l < n; l++) {
            const int c = pb->lmk_obs_ptr[l + 1] - pb->lmk_obs_ptr[l];
            if (c < 0) return "nofov_scale: lmk_obs_ptr is not monotone";
            if (c > NOFOV_PLAN_MAX_OBS_PER_LMK) return "nofov_scale: more than 16 angular factors on a landmark";
            if (pb->scale_cam[l] < 0 || pb->scale_cam[l] >= nc) return "nofov_scale: scale_cam out of range";
        }
    } else if (no != 0) return "nofov_scale: observations without landmarks";
    for (int o = 0; o < no; o++)
        if (pb->obs_frame[o] < 0 || pb->obs_frame[o] >= nfr || pb->obs_cam[o] < 0 || pb->obs_cam[o] >= nc) return "nofov_scale: observation index out of range";
    fixed = pb->fix_scale < 0 ? nofov_reference_fix_scale(pb->T_cam0_cam0p) : pb->fix_scale;
    if (n == 0 && fixed) return "nofov_scale: no landmark and a constant scale: nothing to solve";
    return nullptr;
}

// constant tables: a zero-delta pose table per frame (angular_factor), A | b0 | v per camera (scale factor).
// ftab: NOFOV_PLAN_FTAB doubles per frame, ctab: NOFOV_PLAN_CTAB doubles per camera
inline void nofov_tables(const sadvio_nofov_problem* pb, double* ftab, double* ctab) {
    const double* Tm = pb->T_cam0_cam0p;
    const double I3[9] = {1, 0, 0, 0, 1, 0, 0, 0, 1};
    for (int k = 0; k < pb->n_frames; k++) {
        const double* T = pb->frame_T_f_w + 12 * (size_t)k;
        double* o = &ftab[NOFOV_PLAN_FTAB * (size_t)k];
        memcpy(o, T, 96); memcpy(o + 12, I3, 72); memcpy(o + 21, T, 72); memcpy(o + 30, I3, 72);
    }
    auto mul = [](const double* A, const double* B, double* C) {   // C = A B (3 x 3 row-major)
        for (int i = 0; i < 3; i++) for (int j = 0; j < 3; j++) C[3 * i + j] = A[3 * i] * B[j] + A[3 * i + 1] * B[3 + j] + A[3 * i + 2] * B[6 + j];
    };
    auto mv = [](const double* A, const double* x, double* y) { for (int i = 0; i < 3; i++) y[i] = A[3 * i] * x[0] + A[3 * i + 1] * x[1] + A[3 * i + 2] * x[2]; };
    const double* T0 = pb->cam_T_s_f + 12 * (size_t)pb->cam0;
    const double* Tf = pb->frame_T_f_w;
    double Rcw[9], tcw[3], R0t[9], Rt[9];
    mul(T0, Tf, Rcw); mv(T0, Tf + 9, tcw);
    for (int a = 0; a < 3; a++) tcw[a] += T0[9 + a];                               // T_cam0_w = T_s_f(cam0) T_f_w(f)
    for (int i = 0; i < 3; i++) for (int j = 0; j < 3; j++) { R0t[3 * i + j] = T0[3 * j + i]; Rt[3 * i + j] = Tm[3 * j + i]; }
    for (int c = 0; c < pb->n_cam; c++) {
        const double* Ts = pb->cam_T_s_f + 12 * (size_t)c;
        double Rc[9], tc[3], q[3], B[9];
        mul(Ts, R0t, Rc); mv(Rc, T0 + 9, q);
        for (int a = 0; a < 3; a++) tc[a] = Ts[9 + a] - q[a];                         // T_cam_cam0 = T_s_f(c) T_s_f(cam0)^-1
        mul(Rc, Rt, B);                                                               // Rc R^T
        double* o = &ctab[NOFOV_PLAN_CTAB * (size_t)c];
        mul(B, Rcw, o);
        mv(B, tcw, o + 9);
        for (int a = 0; a < 3; a++) o[9 + a] += tc[a];
        mv(B, Tm + 9, o + 12);
    }
}
