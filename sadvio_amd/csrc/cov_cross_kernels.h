// cov_cross_kernels.h — sadvio_ba_covariance_cross, device side: the cross block Sigma(a, l) between a key-frame and a landmark and
// the innovation covariance of a candidate observation of l in a. Runs behind cov_kernels.h's assembly, the inversion and k_cov_lmk
// (cov_cross_driver.h), whose tables it reads and leaves as they are:
//   eliminated landmark   Sigma_al = -sum_{e in obs(l)} Sigma_pp(a, c_e) W_e^T                       (plain assembly: ent_w holds W_e)
//                         Sigma_al = -(sum_e Sigma_pp(a, c_e) C_e^T) R^-T                            (square-root: ent_w holds C_e, hll R)
//   landmark kept in the reduced system   Sigma_pp(a, the landmark's columns)
//   constant key-frame or landmark        zeros;   singular landmark: NaN
// Kernels, in launch order:
//   k_cov_band_rows  band route only: the whole block row Sigma(a, :) of every distinct key-frame asked for, by substitution with L's
//                    band — k_cov_band_cols with the backward sweep carried up to row 0. Every candidate of the band route is served
//                    from these rows (never from Sigma's band), so its bits cannot depend on where its observers lie.
//   k_cov_cross      one workgroup per entry of the plan's workgroup table (cov_cross_plan.h): candidates of ONE key-frame. The
//                    workgroup stages the key-frame's block row (D x N_p doubles, [g][i]) in LDS once and serves its candidates in
//                    passes; one lane per output entry (i, j): 18 lanes per candidate and three candidates per wave for D = 6, 45 of
//                    64 lanes for D = 15. A lane walks its landmark's entries in list order: a fixed order, the same bits whatever
//                    else the call asks for and wherever the candidate stands in it.
//                    LIMIT: a row of more than CovCrossDev::stage_max doubles (COVX_STAGE_MAX = 16 384: 128 KB of the CU's 160 KB; D = 6:
//                    N_p <= 2 730, D = 15: N_p <= 1 092) is not staged; the lanes then read it from global memory (same order, same bits).
//   k_cov_innov      one thread per candidate: the factor at x* (pixel_factor / angular_factor, whitened, no robust loss),
//                    P = J_a Sigma_aa J_a^T + J_a Sigma_al J_l^T + (..)^T + J_l Sigma_ll J_l^T + I in registers, the closed-form 2 x 2
//                    inverse and maha2 = r^T P^-1 r. Sigma_aa comes from the same block row, Sigma_ll from k_cov_lmk's table.
// No floating-point atomics; every sum in a fixed order. Part of the library's single translation unit; not a public header.
#pragma once
#include "cov_band_kernels.h"

namespace sadvio {

constexpr int COVX_THREADS = 256;
constexpr int COVX_STAGE_MAX = 16384;          // doubles of a staged block row
constexpr int COVX_PASSES = 8;                 // passes of a workgroup over its candidates (cov_cross_driver.h sizes the plan with it)
constexpr int covx_per_wave(int D) { return 64 / (3 * D); }
constexpr int covx_per_wg(int D) { return COVX_PASSES * (COVX_THREADS / 64) * covx_per_wave(D); }
// candidate status (include/sadvio_ba.h: SADVIO_CROSS_*)
constexpr int COVX_OK = 0, COVX_LMK_SINGULAR = 1, COVX_PROJ_INVALID = 2;

struct CovCrossDev {
    int n;                   // candidates
    int band;                // rows holds the band route's solved block rows (addressed by row slot), else Sigma_pp (by free index)
    int stage_max;           // doubles of a block row a workgroup stages in LDS
    const double* rows;      // block row r at rows + r * D * N_p, [g][i]
    const int* flag;         // band route: the pivot flag (!= 0: nothing is written); else null
    const int* order;        // [n] the plan's candidate order
    const int* wgs;          // [workgroups][4] free index | first position | one past the last | row slot
    const int* kf;           // [n] request: key-frame of the window
    const int* lmk;          // [n] landmark of the window
    const int* cam;          // [n] GLOBAL camera index (innovation only)
    const int* crow;         // [n] block row of the candidate's key-frame in `rows`, -1: constant (innovation only)
    const double* meas;      // [n][2 | 3] (innovation only)
    double* cross;           // [n][D][3]
    double* innov;           // [n][4]
    double* maha2;           // [n]
    int* status;             // [n] COVX_*
};

// The band route's block rows: X[(x * dpf + g) * n + i] = Sigma[col[x] + g][i] for EVERY i (Sigma is symmetric: the row is the
// solved column). k_cov_band_cols's substitution — one group of 16 lanes per right-hand side, lane q the terms q, q + 16, .. of a
// row's sum, a butterfly: a fixed order — with the backward sweep not stopped at the band's edge but carried to row 0, where
// y = 0 above the key-frame's own block.
__global__ __launch_bounds__(COVBAND_THREADS) void k_cov_band_rows(CovBand B, const int* __restrict__ col, double* __restrict__ X) {
    const int n = B.n, M = B.M, bw = B.bw, dpf = B.dpf, t = threadIdx.x;
    if (*B.flag != 0) return;
    __shared__ double win[COVBAND_THREADS / COVBAND_GROUP][COVBAND_MAXW];
    const int g = t / COVBAND_GROUP, q = t % COVBAND_GROUP;
    const bool act = g < dpf;
    const int cb = col[blockIdx.x];
    double* Xg = X + ((size_t)blockIdx.x * dpf + (act ? g : 0)) * n;
    double* wg = win[g];
    double lv[COVBAND_LV], ld = 0.0;
    auto fetch_f = [&](int i) {
#pragma unroll
        for (int u = 0; u < COVBAND_LV; u++) {
            const int k = i - 1 - q - COVBAND_GROUP * u;
            lv[u] = (i < n && k >= cb && i - k < bw) ? B.Lb[(long long)i * M + (i - k)] : 0.0;
        }
        ld = i < n ? B.Lb[(long long)i * M] : 1.0;
    };
    fetch_f(cb);
    for (int i = cb; i < n; i++) {
        double s = 0.0;
#pragma unroll
        for (int u = 0; u < COVBAND_LV; u++) {
            const int k = i - 1 - q - COVBAND_GROUP * u;
            if (k >= cb && i - k < bw) s += lv[u] * wg[k % M];
        }
        const double d = ld;
        fetch_f(i + 1);
#pragma unroll
        for (int m = COVBAND_GROUP / 2; m > 0; m >>= 1) s += __shfl_xor(s, m, COVBAND_GROUP);
        const double y = ((i == cb + g ? 1.0 : 0.0) - s) / d;
        if (q == 0 && act) { wg[i % M] = y; Xg[i] = y; }
        __syncthreads();
    }
    auto fetch_b = [&](int i) {
#pragma unroll
        for (int u = 0; u < COVBAND_LV; u++) {
            const int k = i + 1 + q + COVBAND_GROUP * u;
            lv[u] = (i >= 0 && k < n && k - i < bw) ? B.Lb[(long long)k * M + (k - i)] : 0.0;
        }
        ld = i >= 0 ? B.Lb[(long long)i * M] : 1.0;
    };
    fetch_b(n - 1);
    for (int i = n - 1; i >= 0; i--) {
        double s = 0.0;
#pragma unroll
        for (int u = 0; u < COVBAND_LV; u++) {
            const int k = i + 1 + q + COVBAND_GROUP * u;
            if (k < n && k - i < bw) s += lv[u] * wg[k % M];
        }
        const double d = ld;
        fetch_b(i - 1);
#pragma unroll
        for (int m = COVBAND_GROUP / 2; m > 0; m >>= 1) s += __shfl_xor(s, m, COVBAND_GROUP);
        if (q == 0 && act) {
            const double x = ((i >= cb ? Xg[i] : 0.0) - s) / d;
            wg[i % M] = x; Xg[i] = x;
        }
        __syncthreads();
    }
}

// Entry (i, j) of Sigma(a, l) for an eliminated landmark with n entries at e0; row = the key-frame's block row, [g][i]
template <bool SQRT>
__device__ __forceinline__ double covx_entry(const CovDev& C, const double* row, int Np, int l, long long e0, int n, int i, int j) {
    const double* ri = row + (long long)i * Np;
    if (!SQRT) {
        double acc = 0.0;
        for (int e = 0; e < n; e++) {
            const double* s = ri + C.ent_col[e0 + e];
            const double* w = C.ent_w + (e0 + e) * COV_ENT_W + 6 * j;
#pragma unroll
            for (int k = 0; k < 6; k++) acc += s[k] * w[k];
        }
        return 0.0 - acc;
    }
    double T[3] = {0.0, 0.0, 0.0};   // row i of sum_e Sigma_pp(a, c_e) C_e^T
    for (int e = 0; e < n; e++) {
        const double* s = ri + C.ent_col[e0 + e];
        const double* c = C.ent_w + (e0 + e) * COV_ENT_W;
#pragma unroll
        for (int m = 0; m < 3; m++)
#pragma unroll
            for (int k = 0; k < 6; k++) T[m] += s[k] * c[6 * m + k];
    }
    const double* R = C.hll + 6 * (long long)l;   // upper: 00 01 02 11 12 22
    double U[9] = {0, 0, 0, 0, 0, 0, 0, 0, 0};    // R^-1, upper (as k_cov_lmk<G, true>)
    U[0] = 1.0 / R[0]; U[4] = 1.0 / R[3]; U[8] = 1.0 / R[5];
    U[1] = -R[1] * U[4] / R[0];
    U[5] = -R[4] * U[8] / R[3];
    U[2] = -(R[1] * U[5] + R[2] * U[8]) / R[0];
    double acc = 0.0;                             // (T R^-T)[i][j] = sum_{m >= j} T[m] U[j][m]
    for (int m = j; m < 3; m++) acc += T[m] * U[3 * j + m];
    return 0.0 - acc;
}

template <int D, bool SQRT>
__global__ __launch_bounds__(COVX_THREADS) void k_cov_cross(DevPtrs P, CovDev C, CovCrossDev X) {
    extern __shared__ double cx_lds[];
    if (X.flag && *X.flag != 0) return;   // (uniform) the factor is not usable
    const WinDev W = P.win[C.w];
    const int t = threadIdx.x, Np = C.Np;
    const int f = X.wgs[4 * blockIdx.x], p0 = X.wgs[4 * blockIdx.x + 1], p1 = X.wgs[4 * blockIdx.x + 2], slot = X.wgs[4 * blockIdx.x + 3];
    const double* base = f >= 0 ? X.rows + (size_t)(X.band ? slot : f) * D * Np : nullptr;
    const bool staged = f >= 0 && D * Np <= X.stage_max;
    if (staged)
        for (int idx = t; idx < D * Np; idx += COVX_THREADS) cx_lds[idx] = base[idx];
    __syncthreads();
    constexpr int CPW = covx_per_wave(D), PER_PASS = (COVX_THREADS / 64) * CPW;
    const int ln = t & 63, cw = ln / (3 * D), en = ln - cw * 3 * D;
    const int i = en / 3, j = en - 3 * i;
    if (cw >= CPW) return;
    for (int pos = p0 + (t >> 6) * CPW + cw; pos < p1; pos += PER_PASS) {
        const int c = X.order[pos], l = X.lmk[c];
        const int status = C.status[l];
        const int gl = W.lmk_base + l;
        double v = 0.0;
        if (status == COV_LMK_SINGULAR) v = __builtin_nan("");
        else if (f < 0 || status == COV_LMK_CONST) v = 0.0;
        else if (status == COV_LMK_REDUCED) {
            const int lr = P.lmk_red[gl];
            v = staged ? cx_lds[i * Np + lr + j] : base[(long long)i * Np + lr + j];
        } else {
            const long long e0 = P.lmk_ob[gl] - W.obs_base;
            const int n = C.ent_n[l];
            v = staged ? covx_entry<SQRT>(C, cx_lds, Np, l, e0, n, i, j) : covx_entry<SQRT>(C, base, Np, l, e0, n, i, j);
        }
        X.cross[((size_t)c * D + i) * 3 + j] = v;
        if (en == 0) X.status[c] = status == COV_LMK_SINGULAR ? COVX_LMK_SINGULAR : COVX_OK;
    }
}

// The innovation of candidate c. FACTOR 0: pixel_factor (meas uv; a projection that fails Camera::project's tests keeps its
// Jacobians, r = 0, status COVX_PROJ_INVALID); 1: angular_factor (meas a unit bearing). J_a is 2 x 6 on the pose part of the
// key-frame's block.
template <int FACTOR, int D>
__global__ __launch_bounds__(COVX_THREADS) void k_cov_innov(DevPtrs P, CovDev C, CovCrossDev X) {
    if (X.flag && *X.flag != 0) return;
    const WinDev W = P.win[C.w];
    const int c = blockIdx.x * COVX_THREADS + threadIdx.x;
    if (c >= X.n) return;
    const int l = X.lmk[c], gl = W.lmk_base + l;
    const long long gkf = W.kf_base + X.kf[c];
    if (C.status[l] == COV_LMK_SINGULAR) {
        const double nan = __builtin_nan("");
        for (int q = 0; q < 4; q++) X.innov[4 * (size_t)c + q] = nan;
        X.maha2[c] = nan;
        X.status[c] = COVX_LMK_SINGULAR;
        return;
    }
    const double* xl = P.xl + (long long)C.cur * P.xl_stride + 3 * (long long)gl;
    const double pw[3] = {P.lmk_p[3 * (long long)gl] + xl[0], P.lmk_p[3 * (long long)gl + 1] + xl[1], P.lmk_p[3 * (long long)gl + 2] + xl[2]};
    const double* tab = C.ptab + gkf * POSE_TAB;
    const int gc = X.cam[c];
    double r[2], Jp[12], Jl[6];
    bool valid = true;
    if (FACTOR == 0) {
        const double* m = X.meas + 2 * (size_t)c;
        valid = pixel_factor<true>(tab, P.cam_K + 4 * (long long)gc, P.cam_T + 12 * (long long)gc, pw, m[0], m[1], P.cam_isig[gc], r, Jp, Jl);
    } else {
        const double* m = X.meas + 3 * (size_t)c;
        double b[3] = {m[0], m[1], m[2]};
        angular_factor<true>(tab, P.cam_T + 12 * (long long)gc, pw, b, P.cam_isig[gc], r, Jp, Jl);
    }
    double M[4] = {0.0, 0.0, 0.0, 0.0};
    const int cr = X.crow[c];
    if (cr >= 0) {   // J_a Sigma_aa J_a^T, Sigma_aa the pose 6 x 6 of the key-frame's block row
        const int ca = P.kf_fidx[gkf] * D;
        const double* Saa = X.rows + (size_t)cr * D * C.Np + ca;
        for (int a = 0; a < 6; a++) {
            double t0 = 0.0, t1 = 0.0;
#pragma unroll
            for (int b = 0; b < 6; b++) {
                const double s = Saa[(long long)a * C.Np + b];
                t0 += s * Jp[b]; t1 += s * Jp[6 + b];
            }
            M[0] += Jp[a] * t0; M[1] += Jp[a] * t1; M[2] += Jp[6 + a] * t0; M[3] += Jp[6 + a] * t1;
        }
        // J_a Sigma_al J_l^T and its transpose
        const double* Sal = X.cross + (size_t)c * D * 3;
        double A[6] = {0.0, 0.0, 0.0, 0.0, 0.0, 0.0};
        for (int a = 0; a < 6; a++)
#pragma unroll
            for (int j = 0; j < 3; j++) { A[j] += Jp[a] * Sal[3 * a + j]; A[3 + j] += Jp[6 + a] * Sal[3 * a + j]; }
        double X2[4];
        for (int q = 0; q < 2; q++)
            for (int s = 0; s < 2; s++) X2[2 * q + s] = A[3 * q] * Jl[3 * s] + A[3 * q + 1] * Jl[3 * s + 1] + A[3 * q + 2] * Jl[3 * s + 2];
        M[0] += 2.0 * X2[0]; M[1] += X2[1] + X2[2]; M[2] += X2[2] + X2[1]; M[3] += 2.0 * X2[3];
    }
    {   // J_l Sigma_ll J_l^T (zeros for a constant landmark)
        const double* L = C.lout + 9 * (long long)l;
        double B2[6];
        for (int q = 0; q < 2; q++)
            for (int j = 0; j < 3; j++) B2[3 * q + j] = Jl[3 * q] * L[j] + Jl[3 * q + 1] * L[3 + j] + Jl[3 * q + 2] * L[6 + j];
        for (int q = 0; q < 2; q++)
            for (int s = 0; s < 2; s++) M[2 * q + s] += B2[3 * q] * Jl[3 * s] + B2[3 * q + 1] * Jl[3 * s + 1] + B2[3 * q + 2] * Jl[3 * s + 2];
    }
    const double p00 = 1.0 + M[0], p11 = 1.0 + M[3], p01 = 0.5 * (M[1] + M[2]);
    const double det = p00 * p11 - p01 * p01;
    X.innov[4 * (size_t)c] = p00; X.innov[4 * (size_t)c + 1] = p01; X.innov[4 * (size_t)c + 2] = p01; X.innov[4 * (size_t)c + 3] = p11;
    X.maha2[c] = (p11 * r[0] * r[0] - 2.0 * p01 * r[0] * r[1] + p00 * r[1] * r[1]) / det;
    X.status[c] = valid ? COVX_OK : COVX_PROJ_INVALID;
}

}  // namespace sadvio
