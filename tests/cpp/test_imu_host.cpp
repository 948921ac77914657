// Stand-alone check of sadvio_amd/csrc/imu_host.h (host only; built and run by tests/test_capi_host_cpu.py):
//   imu_sqrt_information  on a covariance whose elimination swaps rows, on a diagonal one, and on two that must be refused (a zero
//                         column, a symmetric matrix with one negative eigenvalue): W upper triangular, W^T W cov = I, W equal to
//                         the oracle's function of the same name (oracle/factors.h)
//   host_exp_so3          at |(a, b)| = 0, 1e-10, 1e-8 (the two sides of the first-order branch at 1e-9), 1 and pi - 1e-6: Rodrigues'
//                         formula in long double to 16 eps; below the threshold I + [v]x exactly
//   make_imu_dev          carries the factor's fields into the device record
// The bars of the first two W checks are 8 x what the same function gave for these matrices before it moved into the header (it was
// moved, not rewritten: the margin covers the compiler only). Measured then, g++ -O1 and hipcc's host pass alike:
//   swap:     |W^T W cov - I|_max = 1.776e-15   |W - W_oracle|_max = 0
//   diagonal: |W^T W cov - I|_max = 2.220e-16   |W - W_oracle|_max = 0
#include <cfloat>
#include <cmath>
#include <cstdio>
#include <cstring>

#include "../../sadvio_amd/csrc/imu_host.h"

namespace oracle_ref {
#include "../../oracle/factors.h"
}

static const double BAR_INVERSE[2] = {8 * 1.776e-15, 8 * 2.220e-16};
static const double BAR_ORACLE[2] = {8 * 0.0, 8 * 0.0};

static int fails = 0;
#define CHECK(cond, ...) do { if (!(cond)) { fails++; printf("MISMATCH %s:%d: ", __FILE__, __LINE__); printf(__VA_ARGS__); printf("\n"); } } while (0)

static void cov_swap(double* C) {   // |C[1][0]| = 2 > C[0][0] = 1: the first column's pivot is row 1
    memset(C, 0, 81 * sizeof(double));
    for (int i = 0; i < 9; i++) C[10 * i] = 0.5 * (i + 1);
    C[0] = 1.0; C[1] = C[9] = 2.0; C[10] = 5.0;
    C[2] = C[18] = 0.3;
    C[3 * 9 + 8] = C[8 * 9 + 3] = -0.2;
}
static void cov_diag(double* C) {
    memset(C, 0, 81 * sizeof(double));
    for (int i = 0; i < 9; i++) C[10 * i] = 1e-6 * (i + 1) * (i + 1);
}

static void check_w(int which, const double* C) {
    double W[81], Wo[81];
    const bool ok = imu_sqrt_information(C, W);
    CHECK(ok, "case %d refused", which);
    CHECK(oracle_ref::imu_sqrt_information(C, Wo) == 0, "case %d: the oracle refuses", which);
    if (!ok) return;
    for (int i = 0; i < 9; i++)
        for (int j = 0; j < i; j++) CHECK(W[9 * i + j] == 0.0, "case %d: W[%d][%d] = %g below the diagonal", which, i, j, W[9 * i + j]);
    double inv = 0.0, orc = 0.0;
    for (int i = 0; i < 9; i++)
        for (int j = 0; j < 9; j++) {
            double s = 0.0;   // (W^T W cov)[i][j]
            for (int k = 0; k < 9; k++) {
                double wtw = 0.0;
                for (int q = 0; q < 9; q++) wtw += W[9 * q + i] * W[9 * q + k];
                s += wtw * C[9 * k + j];
            }
            inv = std::fmax(inv, std::fabs(s - (i == j ? 1.0 : 0.0)));
            orc = std::fmax(orc, std::fabs(W[9 * i + j] - Wo[9 * i + j]));
        }
    printf("case %d: |W^T W cov - I|_max = %.3e (bar %.3e)   |W - W_oracle|_max = %.3e (bar %.3e)\n", which, inv, BAR_INVERSE[which], orc, BAR_ORACLE[which]);
    CHECK(inv <= BAR_INVERSE[which], "case %d: W^T W cov is not the identity", which);
    CHECK(orc <= BAR_ORACLE[which], "case %d: W differs from the oracle's", which);
}

static void check_exp(double th) {
    const double a = 0.6 * th, b = 0.8 * th;
    double R[9];
    host_exp_so3(a, b, R);
    const long double la = a, lb = b, lt = sqrtl(la * la + lb * lb);
    const long double S[9] = {0, 0, lb, 0, 0, -la, -lb, la, 0};
    const long double f1 = lt > 0 ? sinl(lt) / lt : 1.0L, f2 = lt > 0 ? (1.0L - cosl(lt)) / (lt * lt) : 0.5L;
    double worst = 0.0;
    for (int i = 0; i < 3; i++)
        for (int j = 0; j < 3; j++) {
            long double s2 = 0;
            for (int k = 0; k < 3; k++) s2 += S[3 * i + k] * S[3 * k + j];
            const long double ref = (i == j ? 1.0L : 0.0L) + f1 * S[3 * i + j] + f2 * s2;
            worst = std::fmax(worst, (double)fabsl((long double)R[3 * i + j] - ref));
        }
    printf("exp_so3 at |v| = %.17g: max error %.3e (bar %.3e)\n", th, worst, 16 * DBL_EPSILON);
    CHECK(worst <= 16 * DBL_EPSILON, "exp_so3 at |v| = %g is off Rodrigues' formula", th);
    if (std::sqrt(a * a + b * b) < 1e-9) {
        const double F[9] = {1, 0, b, 0, 1, -a, -b, a, 1};
        for (int i = 0; i < 9; i++) CHECK(R[i] == F[i], "exp_so3 at |v| = %g: entry %d is not first order", th, i);
    }
}

int main() {
    double C[81], W[81];
    cov_swap(C); check_w(0, C);
    cov_diag(C); check_w(1, C);
    cov_diag(C);
    for (int i = 0; i < 9; i++) C[9 * i + 4] = C[9 * 4 + i] = 0.0;
    CHECK(!imu_sqrt_information(C, W), "a covariance with a zero column is accepted");
    cov_diag(C);
    C[10 * 5] = -1.0;
    CHECK(!imu_sqrt_information(C, W), "a matrix with a negative eigenvalue is accepted");

    const double pi = 3.14159265358979323846;
    for (double th : {0.0, 1e-10, 1e-8, 1.0, pi - 1e-6}) check_exp(th);

    sadvio_imu_factor f;
    memset(&f, 0, sizeof(f));
    f.kf_i = 2; f.kf_j = 3; f.dt = 0.25; f.bacc_noise = 2.0; f.bgyr_noise = 4.0;
    for (int i = 0; i < 9; i++) { f.delta_R[i] = 1 + i; f.J_dR_bg[i] = 10 + i; f.J_dv_ba[i] = 20 + i; f.J_dv_bg[i] = 30 + i; f.J_dp_ba[i] = 40 + i; f.J_dp_bg[i] = 50 + i; }
    for (int i = 0; i < 3; i++) { f.delta_v[i] = 60 + i; f.delta_p[i] = 70 + i; }
    cov_swap(f.cov);
    ImuDev o;
    memset(&o, 0xff, sizeof(o));
    CHECK(make_imu_dev(f, 100, o), "make_imu_dev refuses a positive definite covariance");
    imu_sqrt_information(f.cov, W);
    CHECK(o.kf_i == 102 && o.kf_j == 103 && o.dt == 0.25 && o.win == 0 && o.pad == 0 && o.sa == 1.0 && o.sg == 0.5, "make_imu_dev: header fields");
    CHECK(!memcmp(o.dR, f.delta_R, 72) && !memcmp(o.dv, f.delta_v, 24) && !memcmp(o.dp, f.delta_p, 24) && !memcmp(o.J_dR_bg, f.J_dR_bg, 72) &&
          !memcmp(o.J_dv_ba, f.J_dv_ba, 72) && !memcmp(o.J_dv_bg, f.J_dv_bg, 72) && !memcmp(o.J_dp_ba, f.J_dp_ba, 72) && !memcmp(o.J_dp_bg, f.J_dp_bg, 72) &&
          !memcmp(o.W, W, sizeof(W)), "make_imu_dev: arrays");
    f.cov[10 * 5] = -1.0;
    CHECK(!make_imu_dev(f, 0, o), "make_imu_dev accepts an indefinite covariance");

    printf(fails ? "%d checks failed\n" : "OK\n", fails);
    return fails ? 1 : 0;
}
