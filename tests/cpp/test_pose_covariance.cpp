// pose_covariance_jacobian / pose_covariance_ros (include/sadvio_optimizer.hpp) against central finite differences of the
// composition they linearise: T_f_w' = T_f_w (exp(w), tau) (geometry.h:198-203), T_w_f' = T_f_w'^-1, position error c' - c and
// orientation error theta with R_w_f' = exp(theta) R_w_f. Stand-alone: prints OK and returns 0, or says what differs.
#include <cmath>
#include <cstdio>
#include <random>

#include "sadvio_optimizer.hpp"

using namespace sadvio;

static void error_of(const Pose& T_f_w, const double* d6, double* e6) {
    Pose Tp = T_f_w;
    apply_pose_delta(Tp, d6);
    const Pose A = pose_inv(T_f_w), B = pose_inv(Tp);
    for (int i = 0; i < 3; i++) e6[i] = B.t[i] - A.t[i];
    double M[9];   // R_w_f' R_w_f^T = exp(theta); theta = vee of its skew part (sin|theta| / |theta| = 1 - O(h^2))
    for (int i = 0; i < 3; i++)
        for (int j = 0; j < 3; j++) M[3 * i + j] = B.R[3 * i] * A.R[3 * j] + B.R[3 * i + 1] * A.R[3 * j + 1] + B.R[3 * i + 2] * A.R[3 * j + 2];
    e6[3] = 0.5 * (M[7] - M[5]); e6[4] = 0.5 * (M[2] - M[6]); e6[5] = 0.5 * (M[3] - M[1]);
}

int main() {
    std::mt19937 rng(7);
    std::normal_distribution<double> N(0.0, 1.0);
    double worst = 0.0;
    for (int trial = 0; trial < 20; trial++) {
        Pose T;
        double w[3] = {N(rng), N(rng), N(rng)};
        exp_so3(w, T.R);
        for (int i = 0; i < 3; i++) T.t[i] = 5.0 * N(rng);
        double Jm[36];
        pose_covariance_jacobian(T, Jm);
        const double h = 1e-6;
        for (int k = 0; k < 6; k++) {
            double dp[6] = {0, 0, 0, 0, 0, 0}, dm[6] = {0, 0, 0, 0, 0, 0}, ep[6], em[6];
            dp[k] = h; dm[k] = -h;
            error_of(T, dp, ep); error_of(T, dm, em);
            for (int i = 0; i < 6; i++) worst = std::fmax(worst, std::fabs((ep[i] - em[i]) / (2 * h) - Jm[6 * i + k]));
        }
        // cov_ros = Jm cov Jm^T on a random symmetric positive definite block: symmetric, and equal to the plain triple product
        double A[36], cov[36], out[36];
        for (int i = 0; i < 36; i++) A[i] = N(rng);
        for (int i = 0; i < 6; i++)
            for (int j = 0; j < 6; j++) { double v = i == j ? 1e-3 : 0.0; for (int k = 0; k < 6; k++) v += A[6 * i + k] * A[6 * j + k]; cov[6 * i + j] = 1e-4 * v; }
        pose_covariance_ros(T, cov, out);
        for (int i = 0; i < 6; i++)
            for (int j = 0; j < 6; j++) {
                double v = 0.0;
                for (int a = 0; a < 6; a++) for (int b = 0; b < 6; b++) v += Jm[6 * i + a] * cov[6 * a + b] * Jm[6 * j + b];
                if (std::fabs(out[6 * i + j] - v) > 1e-12 * (1.0 + std::fabs(v)) || std::fabs(out[6 * i + j] - out[6 * j + i]) > 1e-15 * (1.0 + std::fabs(v))) {
                    std::printf("pose_covariance_ros differs at (%d, %d): %.17g against %.17g\n", i, j, out[6 * i + j], v);
                    return 1;
                }
            }
        if (!(out[0] > 0 && out[7] > 0 && out[14] > 0 && out[21] > 0 && out[28] > 0 && out[35] > 0)) { std::printf("non-positive variance\n"); return 1; }
    }
    std::printf("worst |finite difference - Jm| = %.3e\n", worst);
    if (!(worst < 1e-8)) { std::printf("the Jacobian differs from its finite differences\n"); return 1; }
    std::printf("OK\n");
    return 0;
}
