// imu_host.h — host arithmetic of the IMU factors: the square-root information of a preintegration covariance, exp_so3 of a
// two-vector and the device record of one factor. Plain C++17 without the HIP runtime or the handle, so it runs on a machine without
// a GPU (tests/cpp/test_imu_host.cpp). Used by set_imu_factors (factors_driver.h), marginalize (marg_driver.h) and vi_init
// (viinit_driver.h).
#pragma once
#include <cmath>
#include <cstring>
#include <utility>

#include "../../include/sadvio_ba.h"
#include "ba_types.h"

using namespace sadvio;

// 9x9 square-root information W = L^T with L L^T = cov^-1 (residuals.hpp:151-154): Gauss-Jordan inverse with
// partial pivoting + Cholesky, on the host, once per factor.
static bool imu_sqrt_information(const double* cov, double* W) {
    double A[81], I[81];
    memcpy(A, cov, sizeof(A));
    memset(I, 0, sizeof(I));
    for (int i = 0; i < 9; i++) I[i * 9 + i] = 1.0;
    for (int c = 0; c < 9; c++) {
        int piv = c;
        double best = fabs(A[c * 9 + c]);
        for (int r = c + 1; r < 9; r++)
            if (fabs(A[r * 9 + c]) > best) { best = fabs(A[r * 9 + c]); piv = r; }
        if (best == 0.0) return false;
        if (piv != c)
            for (int j = 0; j < 9; j++) { std::swap(A[c * 9 + j], A[piv * 9 + j]); std::swap(I[c * 9 + j], I[piv * 9 + j]); }
        double d = 1.0 / A[c * 9 + c];
        for (int j = 0; j < 9; j++) { A[c * 9 + j] *= d; I[c * 9 + j] *= d; }
        for (int r = 0; r < 9; r++) {
            if (r == c) continue;
            double f = A[r * 9 + c];
            if (f == 0.0) continue;
            for (int j = 0; j < 9; j++) { A[r * 9 + j] -= f * A[c * 9 + j]; I[r * 9 + j] -= f * I[c * 9 + j]; }
        }
    }
    double L[81];
    memset(L, 0, sizeof(L));
    for (int j = 0; j < 9; j++) {
        double s = I[j * 9 + j];
        for (int k = 0; k < j; k++) s -= L[j * 9 + k] * L[j * 9 + k];
        if (!(s > 0.0)) return false;
        double d = sqrt(s);
        L[j * 9 + j] = d;
        for (int i = j + 1; i < 9; i++) {
            double t = I[i * 9 + j];
            for (int k = 0; k < j; k++) t -= L[i * 9 + k] * L[j * 9 + k];
            L[i * 9 + j] = t / d;
        }
    }
    for (int i = 0; i < 9; i++)
        for (int j = 0; j < 9; j++) W[i * 9 + j] = L[j * 9 + i];
    return true;
}

// exp_so3((a, b, 0)) row-major (geometry.h:131-147: first order below 1e-9)
static void host_exp_so3(double a, double b, double* R) {
    const double th = std::sqrt(a * a + b * b);
    const double I[9] = {1, 0, 0, 0, 1, 0, 0, 0, 1};
    if (th < 1e-9) { const double S[9] = {0, 0, b, 0, 0, -a, -b, a, 0}; for (int i = 0; i < 9; i++) R[i] = I[i] + S[i]; return; }
    const double x = a / th, y = b / th;
    const double S[9] = {0, 0, y, 0, 0, -x, -y, x, 0};
    double S2[9];
    for (int i = 0; i < 3; i++) for (int j = 0; j < 3; j++) S2[3 * i + j] = S[3 * i] * S[j] + S[3 * i + 1] * S[3 + j] + S[3 * i + 2] * S[6 + j];
    for (int i = 0; i < 9; i++) R[i] = I[i] + (1.0 - std::cos(th)) * S2[i] + std::sin(th) * S[i];
}
static bool make_imu_dev(const sadvio_imu_factor& f, int kf_base, ImuDev& o) {
    o.kf_i = kf_base + f.kf_i; o.kf_j = kf_base + f.kf_j; o.dt = f.dt;
    memcpy(o.dR, f.delta_R, sizeof(o.dR)); memcpy(o.dv, f.delta_v, sizeof(o.dv)); memcpy(o.dp, f.delta_p, sizeof(o.dp));
    memcpy(o.J_dR_bg, f.J_dR_bg, 72); memcpy(o.J_dv_ba, f.J_dv_ba, 72); memcpy(o.J_dv_bg, f.J_dv_bg, 72);
    memcpy(o.J_dp_ba, f.J_dp_ba, 72); memcpy(o.J_dp_bg, f.J_dp_bg, 72);
    if (!imu_sqrt_information(f.cov, o.W)) return false;
    o.sa = 1.0 / sqrt(f.dt * f.bacc_noise * f.bacc_noise);
    o.sg = 1.0 / sqrt(f.dt * f.bgyr_noise * f.bgyr_noise);
    o.win = 0; o.pad = 0;
    return true;
}
