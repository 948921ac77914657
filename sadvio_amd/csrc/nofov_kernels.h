// nofov_kernels.h — the metric-scale solve of the non-overlapping field-of-view pipeline
// (AngularAdjustmentCERESAnalytic::landmarkOptimizationNoFov, AngularAdjustmentCERESAnalytic.cpp:741-907) on the device.
//
// Unknowns: the scale lambda of T_cam0_cam0p's translation (a plain value starting at 1, constant for a degenerate motion,
// :769-772) and one additive delta per landmark; every pose is constant. Per landmark: AngularErrorScaleCam0 on fp's feature
// (…Analytic.h:122-194, depends on (lambda, dl)) and AngularErrCeres_pointxd_dx on f's and every other key-frame's feature
// (dl only), all under Huber; plus scalePrior(info) on lambda (residuals.hpp:702-717, no loss).
//
// The normal equations are an arrowhead: a 3 x 3 block per landmark, a 3-vector coupling it to lambda and a scalar for lambda.
// The whole LM solve is ONE launch of ONE workgroup, as k_viinit: each thread owns the landmarks l = t, t + T, ..., linearises
// their blocks (loss through Ceres' corrector, huber_rho), forms (H_ll + D_l)^-1 from a 3 x 3 Cholesky and adds the landmark's
// Schur term to the lambda equation; a fixed-order workgroup tree reduces it (and the cost, the model cost change, the norms
// and the gradient max), lambda is solved, every landmark back-substitutes. No floating-point atomics: results are bit-identical
// from run to run. The Ceres-2.2 trust-region rules are those of lm_decide / k_viinit; Ceres' x_norm includes lambda's value.
// Per-landmark state (two linearisations, two iterates, the Jacobi scale) lives in an HBM scratch of NOFOV_LS doubles each.
#pragma once
#include "ba_types.h"
#include "device_math.h"

namespace sadvio {

constexpr int NOFOV_THREADS = 512;
constexpr int NOFOV_MAX_LMK = 65536;         // the reference's test: 10 000 points
constexpr int NOFOV_MAX_OBS_PER_LMK = 16;    // fixed-pose angular factors of one landmark (f + feats)
constexpr int NOFOV_FTAB = 39;               // angular_factor's pose table at a zero delta: R | t | Jr = I | R0 | dR = I
constexpr int NOFOV_CTAB = 15;               // scale factor of one camera: A (9) | b0 (3) | v (3), t_s = A p + b0 - lambda v
constexpr int NOFOV_LIN = 14;                // H_ll (6, packed lower) | g_l (3) | c_l (3) | Jlam^T Jlam | Jlam^T r
constexpr int NOFOV_LS = 40;                 // scratch per landmark: lin[2][14] | x[2][3] | sc[3] | pad
constexpr int NOFOV_OUT = 5;                 // per landmark: dl (3) | gate norm | inlier
constexpr int NOFOV_SUM = 8;                 // initial_cost final_cost radius iterations termination n_success n_unsuccess lambda

struct NoFovDev {
    int n_lmk, fixed, pad0, pad1;
    double info, gate, huber_a;
    const double* ftab;    // [n_frames][NOFOV_FTAB]
    const double* ftsf;    // [n_cam][12] T_s_f
    const double* ctab;    // [n_cam][NOFOV_CTAB]
    const double* lmk_p;   // [n_lmk][3]
    const double* sbear;   // [n_lmk][3] featp's bearing
    const int* scam;       // [n_lmk]
    const int* optr;       // [n_lmk + 1]
    const int* ofr;        // [n_obs]
    const int* ocam;       // [n_obs]
    const double* obear;   // [n_obs][3]
    double* scratch;       // [n_lmk][NOFOV_LS]
    double* out;           // [n_lmk][NOFOV_OUT] | summary [NOFOV_SUM]
    SolveOpts o;
};

// AngularErrorScaleCam0::Evaluate (…Analytic.h:131-189), weight 1 / sigma^2 with sigma = 1. With R, t = T_cam0_cam0p and
// T_cam_cam0 = (Rc, tc): t_s = Rc R^T (T_cam0_w p - lambda t) + tc = A p + b0 - lambda v; d/dlambda = -Je v, d/dp = Je A.
template <bool WANT_J>
__device__ __forceinline__ void nofov_scale_factor(const double* ct, const double* pw, double lam, const double* b, double* r,
                                                   double* Jlam, double* Jl) {
    double ts[3];
    m3_vec(ct, pw, ts);
    for (int a = 0; a < 3; a++) ts[a] += ct[9 + a] - lam * ct[12 + a];
    const double inrm = 1.0 / v3_norm(ts);
    const double bs[3] = {ts[0] * inrm, ts[1] * inrm, ts[2] * inrm};
    const double d[3] = {b[0] - 1, b[1], b[2]};
    double b1[3];
    if (v3_norm(d) > 1e-5) { b1[0] = 0; b1[1] = b[2]; b1[2] = -b[1]; }   // b x (1, 0, 0)
    else { b1[0] = b[1]; b1[1] = -b[0]; b1[2] = 0; }                       // b x (0, 0, 1)
    const double n1 = 1.0 / v3_norm(b1);
    b1[0] *= n1; b1[1] *= n1; b1[2] *= n1;
    double b2[3] = {b1[1] * b[2] - b1[2] * b[1], b1[2] * b[0] - b1[0] * b[2], b1[0] * b[1] - b1[1] * b[0]};
    const double n2 = 1.0 / v3_norm(b2);
    b2[0] *= n2; b2[1] *= n2; b2[2] *= n2;
    const double e[3] = {bs[0] - b[0], bs[1] - b[1], bs[2] - b[2]};
    r[0] = b1[0] * e[0] + b1[1] * e[1] + b1[2] * e[2];
    r[1] = b2[0] * e[0] + b2[1] * e[1] + b2[2] * e[2];
    if (!WANT_J) return;
    const double Pt[6] = {b1[0], b1[1], b1[2], b2[0], b2[1], b2[2]};
    for (int q = 0; q < 2; q++) {
        const double dot = Pt[3 * q] * bs[0] + Pt[3 * q + 1] * bs[1] + Pt[3 * q + 2] * bs[2];
        double je[3];
        for (int j = 0; j < 3; j++) je[j] = (Pt[3 * q + j] - dot * bs[j]) * inrm;
        Jlam[q] = -(je[0] * ct[12] + je[1] * ct[13] + je[2] * ct[14]);
        for (int j = 0; j < 3; j++) Jl[3 * q + j] = je[0] * ct[j] + je[1] * ct[3 + j] + je[2] * ct[6 + j];
    }
}

struct NoFovLm {   // LM state shared by the workgroup (thread 0 writes)
    double radius, decrease_factor, x_cost, x_norm, initial_cost, gmax, lam, sc_lam;
    double h_lam, g_lam;                 // lambda's row of the normal equations at the current linearisation
    double c_cost, c_h, c_g, c_gmax;     // the same at the candidate
    double y_lam;                        // lambda's part of the solution of the damped system
    int iter, n_invalid, n_success, n_unsuccess, termination, done, accepted, fail;
};

// Fixed-order tree over the workgroup of N partial sums per thread (red: [N][NOFOV_THREADS] in LDS); every thread gets the totals.
template <int N>
__device__ __forceinline__ void nofov_sum(double* v, double* red) {
    const int t = threadIdx.x;
    for (int k = 0; k < N; k++) red[k * NOFOV_THREADS + t] = v[k];
    __syncthreads();
    for (int s = NOFOV_THREADS / 2; s > 0; s >>= 1) {
        if (t < s)
            for (int k = 0; k < N; k++) red[k * NOFOV_THREADS + t] += red[k * NOFOV_THREADS + t + s];
        __syncthreads();
    }
    for (int k = 0; k < N; k++) v[k] = red[k * NOFOV_THREADS];
    __syncthreads();
}

__device__ __forceinline__ double nofov_max(double v, double* red) {
    const int t = threadIdx.x;
    red[t] = v;
    __syncthreads();
    for (int s = NOFOV_THREADS / 2; s > 0; s >>= 1) {
        if (t < s) red[t] = fmax(red[t], red[t + s]);
        __syncthreads();
    }
    const double r = red[0];
    __syncthreads();
    return r;
}

__device__ __forceinline__ void nofov_acc(double* lin, const double* r, const double* Jl, const double* Jlam, bool with_lam) {
    for (int q = 0; q < 2; q++) {
        const double* j = Jl + 3 * q;
        lin[0] += j[0] * j[0]; lin[1] += j[1] * j[0]; lin[2] += j[1] * j[1];
        lin[3] += j[2] * j[0]; lin[4] += j[2] * j[1]; lin[5] += j[2] * j[2];
        for (int a = 0; a < 3; a++) lin[6 + a] += j[a] * r[q];
        if (with_lam) {
            for (int a = 0; a < 3; a++) lin[9 + a] += j[a] * Jlam[q];
            lin[12] += Jlam[q] * Jlam[q];
            lin[13] += Jlam[q] * r[q];
        }
    }
}

// Linearise every landmark of this thread at (lam, x[slot]) into lin[slot]; returns per-thread partials
// acc = {sum rho, sum Jlam^T Jlam, sum Jlam^T r} and max |g_l|. FIRST also stores the Jacobi scale of each landmark column.
template <bool FIRST>
__device__ void nofov_linearize(const NoFovDev& P, double lam, int slot, double* acc, double& gm) {
    const bool with_lam = !P.fixed;
    for (int l = threadIdx.x; l < P.n_lmk; l += NOFOV_THREADS) {
        double* S = P.scratch + (long long)l * NOFOV_LS;
        const double* x = S + 2 * NOFOV_LIN + 3 * slot;
        const double pw[3] = {P.lmk_p[3 * l] + x[0], P.lmk_p[3 * l + 1] + x[1], P.lmk_p[3 * l + 2] + x[2]};
        double lin[NOFOV_LIN];
        for (int k = 0; k < NOFOV_LIN; k++) lin[k] = 0.0;
        double rho_sum = 0.0, r[2], Jl[6], Jlam[2], Jp[12], sc;
        nofov_scale_factor<true>(P.ctab + NOFOV_CTAB * P.scam[l], pw, lam, P.sbear + 3 * l, r, Jlam, Jl);
        rho_sum += huber_rho(P.huber_a, r[0] * r[0] + r[1] * r[1], sc);
        for (int q = 0; q < 2; q++) { r[q] *= sc; Jlam[q] *= sc; }
        for (int k = 0; k < 6; k++) Jl[k] *= sc;
        nofov_acc(lin, r, Jl, Jlam, with_lam);
        for (int o = P.optr[l]; o < P.optr[l + 1]; o++) {   // AngularErrCeres_pointxd_dx, constant pose, sigma = 1
            angular_factor<true>(P.ftab + NOFOV_FTAB * P.ofr[o], P.ftsf + 12 * P.ocam[o], pw, P.obear + 3 * (long long)o, 1.0, r, Jp, Jl);
            rho_sum += huber_rho(P.huber_a, r[0] * r[0] + r[1] * r[1], sc);
            for (int q = 0; q < 2; q++) r[q] *= sc;
            for (int k = 0; k < 6; k++) Jl[k] *= sc;
            nofov_acc(lin, r, Jl, Jlam, false);
        }
        double* L = S + NOFOV_LIN * slot;
        for (int k = 0; k < NOFOV_LIN; k++) L[k] = lin[k];
        acc[0] += rho_sum; acc[1] += lin[12]; acc[2] += lin[13];
        gm = fmax(gm, fmax(fabs(lin[6]), fmax(fabs(lin[7]), fabs(lin[8]))));
        if (FIRST) {
            double* s = S + 2 * NOFOV_LIN + 6;
            s[0] = P.o.jacobi_scaling ? 1.0 / (1.0 + sqrt(lin[0])) : 1.0;
            s[1] = P.o.jacobi_scaling ? 1.0 / (1.0 + sqrt(lin[2])) : 1.0;
            s[2] = P.o.jacobi_scaling ? 1.0 / (1.0 + sqrt(lin[5])) : 1.0;
        }
    }
}

// Lower Cholesky factor of H_ll + D_l (D from the Jacobi-scaled diagonal, LM clamps, / radius); false if not SPD.
__device__ __forceinline__ bool nofov_chol(const double* H, const double* sc, double radius, const SolveOpts& o, double* L) {
    double M[6] = {H[0], H[1], H[2], H[3], H[4], H[5]};
    const int dg[3] = {0, 2, 5};
    for (int i = 0; i < 3; i++) {
        const double s2 = sc[i] * sc[i];
        M[dg[i]] += fmin(fmax(s2 * H[dg[i]], o.min_lm_diagonal), o.max_lm_diagonal) / radius / s2;
    }
    if (!(M[0] > 0.0)) return false;
    L[0] = sqrt(M[0]);
    L[1] = M[1] / L[0]; L[3] = M[3] / L[0];
    const double d1 = M[2] - L[1] * L[1];
    if (!(d1 > 0.0)) return false;
    L[2] = sqrt(d1);
    L[4] = (M[4] - L[3] * L[1]) / L[2];
    const double d2 = M[5] - L[3] * L[3] - L[4] * L[4];
    if (!(d2 > 0.0)) return false;
    L[5] = sqrt(d2);
    return isfinite(L[5]) && isfinite(L[4]) && isfinite(L[3]);
}
__device__ __forceinline__ void nofov_fwd(const double* L, const double* b, double* z) {   // L z = b
    z[0] = b[0] / L[0];
    z[1] = (b[1] - L[1] * z[0]) / L[2];
    z[2] = (b[2] - L[3] * z[0] - L[4] * z[1]) / L[5];
}
__device__ __forceinline__ void nofov_bwd(const double* L, const double* z, double* y) {   // L^T y = z
    y[2] = z[2] / L[5];
    y[1] = (z[1] - L[4] * y[2]) / L[2];
    y[0] = (z[0] - L[1] * y[1] - L[3] * y[2]) / L[0];
}

__global__ void __launch_bounds__(NOFOV_THREADS) k_nofov(const NoFovDev* Pp) {
    __shared__ NoFovLm lm;
    __shared__ double red[4 * NOFOV_THREADS];
    const NoFovDev P = *Pp;
    const SolveOpts o = P.o;
    const int t = threadIdx.x, n = P.n_lmk;
    const bool with_lam = !P.fixed;
    for (int l = t; l < n; l += NOFOV_THREADS) {
        double* x = P.scratch + (long long)l * NOFOV_LS + 2 * NOFOV_LIN;
        for (int k = 0; k < 6; k++) x[k] = 0.0;
    }
    if (t == 0) {
        lm.radius = o.initial_radius; lm.decrease_factor = 2.0; lm.lam = 1.0;
        lm.x_norm = with_lam ? 1.0 : 0.0;   // Ceres' x_norm is |x| of the program's parameters: lambda starts at 1
        lm.iter = 0; lm.n_invalid = 0; lm.n_success = 0; lm.n_unsuccess = 0; lm.termination = 0; lm.done = 0; lm.accepted = 1;
        lm.fail = 0;
    }
    __syncthreads();
    int cur = 0;
    {
        double acc[4] = {0.0, 0.0, 0.0, 0.0}, gm = 0.0;
        nofov_linearize<true>(P, 1.0, 0, acc, gm);
        nofov_sum<3>(acc, red);
        gm = nofov_max(gm, red);
        if (t == 0) {
            const double rp = P.info * (1.0 - lm.lam);   // scalePrior: r = info (1 - lambda), J = -info
            lm.x_cost = 0.5 * (acc[0] + (with_lam ? rp * rp : 0.0));
            lm.initial_cost = lm.x_cost;
            lm.h_lam = acc[1] + P.info * P.info;
            lm.g_lam = acc[2] - P.info * rp;
            lm.sc_lam = o.jacobi_scaling ? 1.0 / (1.0 + sqrt(lm.h_lam)) : 1.0;
            lm.gmax = with_lam ? fmax(gm, fabs(lm.g_lam)) : gm;
        }
        __syncthreads();
    }
    while (true) {
        if (t == 0) {   // FinalizeIterationAndCheckIfMinimizerCanContinue
            if (lm.iter >= o.max_num_iterations) { lm.done = 1; lm.termination = 0; }
            else if (lm.gmax <= o.gradient_tolerance) { lm.done = 1; lm.termination = 3; }
            else if (lm.radius < o.min_radius) { lm.done = 1; lm.termination = 4; }
            lm.fail = 0;
        }
        __syncthreads();
        if (lm.done) break;
        const double radius = lm.radius;
        // ---- pass A: per-landmark damped block, its Schur term on the lambda equation ----
        {
            double acc[2] = {0.0, 0.0}, bad = 0.0;
            for (int l = t; l < n; l += NOFOV_THREADS) {
                const double* S = P.scratch + (long long)l * NOFOV_LS;
                const double* H = S + NOFOV_LIN * cur;
                double L[6];
                if (!nofov_chol(H, S + 2 * NOFOV_LIN + 6, radius, o, L)) { bad = 1.0; continue; }
                if (with_lam) {
                    double zc[3], zg[3];
                    nofov_fwd(L, H + 9, zc);
                    nofov_fwd(L, H + 6, zg);
                    acc[0] += zc[0] * zc[0] + zc[1] * zc[1] + zc[2] * zc[2];
                    acc[1] += zc[0] * zg[0] + zc[1] * zg[1] + zc[2] * zg[2];
                }
            }
            nofov_sum<2>(acc, red);
            bad = nofov_max(bad, red);
            if (t == 0) {
                lm.y_lam = 0.0;
                if (bad > 0.0) lm.fail = 1;
                else if (with_lam) {
                    const double s2 = lm.sc_lam * lm.sc_lam;
                    const double Sl = lm.h_lam + fmin(fmax(s2 * lm.h_lam, o.min_lm_diagonal), o.max_lm_diagonal) / radius / s2 - acc[0];
                    const double y = (lm.g_lam - acc[1]) / Sl;
                    if (!(Sl > 0.0) || !isfinite(y)) lm.fail = 1;
                    else lm.y_lam = y;
                }
            }
            __syncthreads();
        }
        // ---- pass B: back substitution, model cost change, step / candidate norms ----
        double mcc = 0.0, sn2 = 0.0, cn2 = 0.0;
        const double dlam = -lm.y_lam, lam_c = lm.lam + dlam;
        if (!lm.fail) {
            double acc[3] = {0.0, 0.0, 0.0}, bad = 0.0;
            const double y_lam = lm.y_lam;
            for (int l = t; l < n; l += NOFOV_THREADS) {
                double* S = P.scratch + (long long)l * NOFOV_LS;
                const double* H = S + NOFOV_LIN * cur;
                double L[6], b[3], z[3], y[3];
                nofov_chol(H, S + 2 * NOFOV_LIN + 6, radius, o, L);
                for (int a = 0; a < 3; a++) b[a] = H[6 + a] - H[9 + a] * y_lam;
                nofov_fwd(L, b, z);
                nofov_bwd(L, z, y);
                const double d[3] = {-y[0], -y[1], -y[2]};
                if (!isfinite(d[0]) || !isfinite(d[1]) || !isfinite(d[2])) bad = 1.0;
                const double Hd[3] = {H[0] * d[0] + H[1] * d[1] + H[3] * d[2], H[1] * d[0] + H[2] * d[1] + H[4] * d[2],
                                      H[3] * d[0] + H[4] * d[1] + H[5] * d[2]};
                double m = 0.0;
                for (int a = 0; a < 3; a++) m += d[a] * (H[6 + a] + 0.5 * Hd[a] + dlam * H[9 + a]);
                acc[0] += m;
                const double* x = S + 2 * NOFOV_LIN + 3 * cur;
                double* c = S + 2 * NOFOV_LIN + 3 * (1 - cur);
                for (int a = 0; a < 3; a++) {
                    c[a] = x[a] + d[a];
                    acc[1] += d[a] * d[a];
                    acc[2] += c[a] * c[a];
                }
            }
            nofov_sum<3>(acc, red);
            bad = nofov_max(bad, red);
            if (bad > 0.0 || !isfinite(dlam)) { if (t == 0) lm.fail = 1; }
            else {
                mcc = -(acc[0] + dlam * (lm.g_lam + 0.5 * lm.h_lam * dlam));
                sn2 = acc[1] + dlam * dlam;
                cn2 = acc[2] + (with_lam ? lam_c * lam_c : 0.0);
            }
            __syncthreads();
        }
        // ---- the candidate, linearised into the other slot (kept if the step is accepted) ----
        if (!lm.fail && mcc > 0.0) {
            double acc[4] = {0.0, 0.0, 0.0, 0.0}, gm = 0.0;
            nofov_linearize<false>(P, lam_c, 1 - cur, acc, gm);
            nofov_sum<3>(acc, red);
            gm = nofov_max(gm, red);
            if (t == 0) {
                const double rp = P.info * (1.0 - lam_c);
                lm.c_cost = 0.5 * (acc[0] + (with_lam ? rp * rp : 0.0));
                lm.c_h = acc[1] + P.info * P.info;
                lm.c_g = acc[2] - P.info * rp;
                lm.c_gmax = with_lam ? fmax(gm, fabs(lm.c_g)) : gm;
            }
        }
        // ---- Ceres 2.2 TrustRegionMinimizer bookkeeping (lm_decide, k_viinit) ----
        if (t == 0) {
            lm.iter += 1;
            lm.accepted = 0;
            if (lm.fail || !(mcc > 0.0)) {
                lm.n_invalid += 1; lm.n_unsuccess += 1;
                if (lm.n_invalid >= o.max_num_consecutive_invalid_steps) { lm.done = 1; lm.termination = 5; }
                else lm.radius *= 0.5;
            } else {
                lm.n_invalid = 0;
                const double cost_change = lm.x_cost - lm.c_cost;
                if (sqrt(sn2) <= o.parameter_tolerance * (lm.x_norm + o.parameter_tolerance)) { lm.done = 1; lm.termination = 2; }
                else if (fabs(cost_change) <= o.function_tolerance * lm.x_cost) { lm.done = 1; lm.termination = 1; }
                else {
                    const double rel = cost_change / mcc;
                    if (rel > o.min_relative_decrease) {
                        lm.accepted = 1;
                        lm.x_norm = sqrt(cn2); lm.x_cost = lm.c_cost; lm.n_success += 1;
                        if (with_lam) lm.lam = lam_c;
                        lm.h_lam = lm.c_h; lm.g_lam = lm.c_g; lm.gmax = lm.c_gmax;
                        const double tt = 2.0 * rel - 1.0;
                        lm.radius = fmin(o.max_radius, lm.radius / fmax(1.0 / 3.0, 1.0 - tt * tt * tt));
                        lm.decrease_factor = 2.0;
                    } else {
                        lm.radius /= lm.decrease_factor; lm.decrease_factor *= 2.0; lm.n_unsuccess += 1;
                    }
                }
            }
        }
        __syncthreads();
        if (lm.accepted) cur ^= 1;
        if (lm.done) break;
    }
    __syncthreads();
    // ---- the result and the gate of :880-899: the scale factor at the solution, no loss ----
    const double lam = lm.lam;
    for (int l = t; l < n; l += NOFOV_THREADS) {
        const double* x = P.scratch + (long long)l * NOFOV_LS + 2 * NOFOV_LIN + 3 * cur;
        const double pw[3] = {P.lmk_p[3 * l] + x[0], P.lmk_p[3 * l + 1] + x[1], P.lmk_p[3 * l + 2] + x[2]};
        double r[2];
        nofov_scale_factor<false>(P.ctab + NOFOV_CTAB * P.scam[l], pw, lam, P.sbear + 3 * l, r, nullptr, nullptr);
        const double g = sqrt(r[0] * r[0] + r[1] * r[1]);
        double* out = P.out + (long long)l * NOFOV_OUT;
        out[0] = x[0]; out[1] = x[1]; out[2] = x[2]; out[3] = g;
        out[4] = (g > P.gate) ? 0.0 : 1.0;
    }
    if (t == 0) {
        double* s = P.out + (long long)n * NOFOV_OUT;
        s[0] = lm.initial_cost; s[1] = lm.x_cost; s[2] = lm.radius; s[3] = lm.iter; s[4] = lm.termination; s[5] = lm.n_success;
        s[6] = lm.n_unsuccess; s[7] = lm.lam;
    }
}

}  // namespace sadvio
