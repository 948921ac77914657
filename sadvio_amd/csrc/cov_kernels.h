// cov_kernels.h — marginal covariances of a solved window (sadvio_ba_covariance), device side.
//
// At the solve's final accepted state x* (the delta buffer FinalRec::s.cur): H = J^T J over every residual block of the window
// (Gauss-Newton: no LM damping, no Jacobi scaling; the visual factors under the solve's Huber corrector), restricted to the free
// parameters, and blocks of Sigma = H^-1 through the solve's own elimination written once more in plain form:
//   S = H_pp - sum_l H_pl H_ll^-1 H_lp        p = free key-frame states | landmarks kept in the reduced system (WinDev::Np columns)
//   Sigma_pp = S^-1                           (unpivoted Cholesky + triangular inverse of dense_chol.h / marg_kernels.h, cov_driver.h)
//   Sigma_ll = H_ll^-1 + W_l Sigma_pp W_l^T   W_l = H_ll^-1 H_lp, for every eliminated landmark
// Kernels, in launch order:
//   k_cov_tables    pose tables of every key-frame at x*; the status a landmark keeps when no tile lists it
//   k_cov_assemble  one workgroup per landmark tile (the handle's Tile / tile_lmk lists, read only), one thread per landmark: linearises
//                   the landmark's observations with pixel_factor / angular_factor / p2l_pseudo_obs, forms H_ll, H_ll^-1 and, per
//                   observing free key-frame, W (3 x 6) and sum Jp^T Jp (6 x 6), stored compactly at the landmark's observation range
//   k_cov_schur     one workgroup per pair of free key-frames: the 6 x 6 block of S, summed over the landmarks in a FIXED order
//                   (thread-strided partial sums, then a workgroup tree) — no floating-point atomics anywhere in this file, so that two
//                   calls give the same bits. On the band route (cov_band_kernels.h) the pair comes from a table of the in-band
//                   pairs instead of blockIdx: the same sums for fewer pairs
//   k_cov_kept      rows / columns of the landmarks kept in the reduced system (one workgroup, observation after observation)
//   k_cov_factors   PosePriordx, IMUFactor + IMUBiasFactor and the listed sparse-prior factors through the evaluators of
//                   device_math.h / kernels.h (pose_prior_factor, imu_factor_body, sparse_eval): one workgroup, factor after factor
//   k_cov_dense     the dense prior's J^T J (WinDev::dp_off: H, formed at upload) through its column map
//   k_cov_lmk       the landmark blocks: one landmark per group of G lanes (below)
// S and the landmark blocks have a second assembly, the square-root one (k_cov_assemble_sqrt, k_cov_schur_sqrt, k_cov_lmk<G, true>,
// further down): the same quantities without the difference above, for windows with landmarks millimetres from a camera centre.
// cov_driver.h (cov_steps) says which runs.
// Bodies and wrappers: the work of k_cov_tables, k_cov_schur, k_cov_kept, k_cov_factors and k_cov_dense is written once, in a
// __device__ __forceinline__ body (cov_tables_body ... cov_dense_body) that takes DevPtrs, CovDev and WinDev by reference. The
// __global__ k_cov_* below each body is the wrapper of sadvio_ba_covariance (CovDev is a kernel argument, WinDev a local copy);
// cov_batch_kernels.h holds the second wrapper, k_covb_*, which loads CovDev from the call's unit table. What says how a sum is
// ordered or why a step is there stands on the body.
// Two kernels are exceptions and stay two copies of one text each, here and in cov_batch_kernels.h; a change to one copy is made to
// the other. k_cov_assemble: behind a shared body the compiler contracts other products into its fused multiply-adds, and every
// block of both calls moves in the last place (measured on the MI355X with scripts/cov_same_results.py); the copies give the bits
// they always gave. k_cov_lmk: the batch call's copy has no long-track test, and behind the shared body k_covb_lmk ran 0.3 - 0.4 %
// longer on 64 config-2 windows (profiles/r24_cov_shared_bodies.txt).
// Long tracks (landmarks the planner keeps out of the tiles) get their rows of the same tables from k_cov_long and their landmark
// blocks from k_cov_lmk_long (cov_long_kernels.h); every other kernel here reads them like any landmark.
// A landmark whose H_ll is not positive definite (one observation; a pivot within 64 ulps of its diagonal entry) is left out of H
// together with its observations and reported as singular. Part of the library's single translation unit; not a public header.
#pragma once
#include "kernels.h"

namespace sadvio {

constexpr int COV_THREADS = 256;
constexpr int COV_SCHUR_THREADS = 128;        // 128 x 36 partial sums in LDS = 36 KB
constexpr int COV_ENT_W = 18, COV_ENT_HPP = 21;
// landmark status
constexpr int COV_LMK_ELIMINATED = 0, COV_LMK_CONST = 1, COV_LMK_REDUCED = 2, COV_LMK_SINGULAR = 3;

struct CovDev {
    int w, cur;              // window, delta buffer that holds x*
    int Np;                  // columns of the reduced system (leading dimension of S / Sigma_pp)
    double huber_a;          // of the solve
    const double* ptab;      // [n_kf_tot][POSE_TAB] at x*
    // per landmark of the window
    double* hll;             // [n_lmk][6] H_ll, upper row-major (00 01 02 11 12 22)
    double* hinv;            // [n_lmk][6] H_ll^-1
    int* status;             // [n_lmk] COV_LMK_*
    int* ent_n;              // [n_lmk] observing free key-frames
    // per entry: entry e of landmark gl sits at lmk_ob[gl] - obs_base + e
    int* ent_col;            // [n_obs] first reduced column of the key-frame
    double* ent_w;           // [n_obs][18] W (3 x 6 row-major); H_lp until the landmark's block is inverted
    double* ent_hpp;         // [n_obs][21] sum Jp^T Jp, lower
    double* S;               // [Np][Np] full symmetric
    const double* Sig;       // [Np][Np] Sigma_pp
    double* lout;            // [n_lmk][9]
    const int* pair_tab;     // band route: [workgroups of k_cov_schur][2] the in-band key-frame pairs (a, b), a >= b; else null
    int* is_long;            // [n_lmk] 1: a long track, filled by k_cov_long and left to k_cov_lmk_long (cov_long_kernels.h); null: the window has none
};

__device__ __forceinline__ void cov_tables_body(const DevPtrs& P, const CovDev& C, const WinDev& W, double* ptab) {
    const int k = blockIdx.x * blockDim.x + threadIdx.x;
    if (k < W.n_lmk) {   // a landmark no tile lists (no observation) has no information of its own
        const int lc = P.lmk_const ? P.lmk_const[W.lmk_base + k] : 0;
        C.status[k] = lc == 1 ? COV_LMK_CONST : (lc == 2 ? COV_LMK_REDUCED : COV_LMK_SINGULAR);
        C.ent_n[k] = 0;
    }
    if (k >= W.n_kf) return;
    const long long kf = W.kf_base + k;
    double d6[6], T0[12], tab[POSE_TAB];
    for (int i = 0; i < 6; i++) d6[i] = P.xp[(long long)C.cur * P.xp_stride + 6 * kf + i];
    for (int i = 0; i < 12; i++) T0[i] = P.kf_T0[12 * kf + i];
    pose_table_entry(T0, d6, tab);
    for (int i = 0; i < POSE_TAB; i++) ptab[kf * POSE_TAB + i] = tab[i];
}

__global__ void k_cov_tables(DevPtrs P, CovDev C, double* ptab) {
    const WinDev W = P.win[C.w];
    cov_tables_body(P, C, W, ptab);
}

// Jacobians of observation o of landmark position pw at x*, corrected as the solve corrects them (lane_linearize, k_build_kept)
template <int FACTOR>
__device__ __forceinline__ void cov_obs_jacobians(const DevPtrs& P, const CovDev& C, int o, const double* pw, double* Jp, double* Jl) {
    const int kf = P.obs_kf[o], craw = P.obs_cam[o];
    const double* tab = C.ptab + (long long)kf * POSE_TAB;
    double r[2];
    if (craw < 0) {   // one half of a PoseToLandmarkFactor riding the elimination: no loss function on it
        const int code = -1 - craw;
        const SparseDev& f = P.sparse[code >> 1];
        p2l_pseudo_obs<true>(tab, pw, f.delta, f.W, code & 1, r, Jp, Jl);
        return;
    }
    if (FACTOR == 0) {
        const double* m = P.obs_meas + 2 * (long long)o;
        pixel_factor<true>(tab, P.cam_K + 4 * (long long)craw, P.cam_T + 12 * (long long)craw, pw, m[0], m[1], P.cam_isig[craw], r, Jp, Jl);
    } else {
        const double* m = P.obs_meas + 3 * (long long)o;
        double b[3] = {m[0], m[1], m[2]};
        angular_factor<true>(tab, P.cam_T + 12 * (long long)craw, pw, b, P.cam_isig[craw], r, Jp, Jl);
    }
    double sc;
    (void)huber_rho(C.huber_a, r[0] * r[0] + r[1] * r[1], sc);
    if (sc != 1.0) {
        for (int i = 0; i < 12; i++) Jp[i] *= sc;
        for (int i = 0; i < 6; i++) Jl[i] *= sc;
    }
}

// inverse of the symmetric 3 x 3 block a (00 01 02 11 12 22) through its Cholesky factor; false = not positive definite
// (a pivot that is not above 64 ulps of its diagonal entry is rounding noise of a rank-deficient block)
__device__ __forceinline__ bool cov_sym3_inverse(const double* a, double* inv) {
    const double tol = 64.0 * 2.220446049250313e-16;
    if (!(a[0] > 0.0)) return false;
    const double l00 = sqrt(a[0]), l10 = a[1] / l00, l20 = a[2] / l00;
    const double d1 = a[3] - l10 * l10;
    if (!(d1 > tol * a[3])) return false;
    const double l11 = sqrt(d1), l21 = (a[4] - l20 * l10) / l11;
    const double d2 = a[5] - l20 * l20 - l21 * l21;
    if (!(d2 > tol * a[5])) return false;
    const double l22 = sqrt(d2);
    // M = L^-1 (lower), inverse = M^T M
    const double m00 = 1.0 / l00, m11 = 1.0 / l11, m22 = 1.0 / l22;
    const double m10 = -l10 * m00 * m11;
    const double m21 = -l21 * m11 * m22;
    const double m20 = -(l20 * m00 + l21 * m10) * m22;
    inv[0] = m00 * m00 + m10 * m10 + m20 * m20;
    inv[1] = m10 * m11 + m20 * m21;
    inv[2] = m20 * m22;
    inv[3] = m11 * m11 + m21 * m21;
    inv[4] = m21 * m22;
    inv[5] = m22 * m22;
    return isfinite(inv[0]) && isfinite(inv[3]) && isfinite(inv[5]);
}

// y = A x for the symmetric 3 x 3 A (00 01 02 11 12 22)
__device__ __forceinline__ void cov_sym3_vec(const double* A, double x0, double x1, double x2, double* y) {
    y[0] = A[0] * x0 + A[1] * x1 + A[2] * x2;
    y[1] = A[1] * x0 + A[3] * x1 + A[4] * x2;
    y[2] = A[2] * x0 + A[4] * x1 + A[5] * x2;
}

template <int FACTOR>
__global__ __launch_bounds__(COV_THREADS) void k_cov_assemble(DevPtrs P, CovDev C) {
    const WinDev W = P.win[C.w];
    const Tile T = P.tiles[W.tile_begin + blockIdx.x];
    for (int i = threadIdx.x; i < T.n_lmk; i += blockDim.x) {
        const int gl = tile_landmark(T, P.tile_lmk, i);
        const int l = gl - W.lmk_base;
        if (l < 0 || l >= W.n_lmk) continue;
        const int ob = P.lmk_ob[gl], oe = P.lmk_oe[gl];
        const long long e0 = ob - W.obs_base;
        const double* xl = P.xl + (long long)C.cur * P.xl_stride + 3 * (long long)gl;
        const double pw[3] = {P.lmk_p[3 * (long long)gl] + xl[0], P.lmk_p[3 * (long long)gl + 1] + xl[1], P.lmk_p[3 * (long long)gl + 2] + xl[2]};
        const int lc = P.lmk_const ? P.lmk_const[gl] : 0;   // 0 free | 1 constant | 2 kept in the reduced system
        double H[6] = {0, 0, 0, 0, 0, 0};
        int n = 0;
        for (int o = ob; o < oe; o++) {
            double Jp[12], Jl[6];
            cov_obs_jacobians<FACTOR>(P, C, o, pw, Jp, Jl);
            H[0] += Jl[0] * Jl[0] + Jl[3] * Jl[3]; H[1] += Jl[0] * Jl[1] + Jl[3] * Jl[4]; H[2] += Jl[0] * Jl[2] + Jl[3] * Jl[5];
            H[3] += Jl[1] * Jl[1] + Jl[4] * Jl[4]; H[4] += Jl[1] * Jl[2] + Jl[4] * Jl[5]; H[5] += Jl[2] * Jl[2] + Jl[5] * Jl[5];
            const int fi = P.kf_fidx[P.obs_kf[o]];
            if (fi < 0) continue;
            const int col = fi * W.dpf;
            int e = 0;
            while (e < n && C.ent_col[e0 + e] != col) e++;
            double* w18 = C.ent_w + (e0 + e) * COV_ENT_W;
            double* h21 = C.ent_hpp + (e0 + e) * COV_ENT_HPP;
            if (e == n) {
                n++;
                C.ent_col[e0 + e] = col;
                for (int q = 0; q < COV_ENT_W; q++) w18[q] = 0.0;
                for (int q = 0; q < COV_ENT_HPP; q++) h21[q] = 0.0;
            }
            for (int a = 0; a < 3; a++)
                for (int c = 0; c < 6; c++) w18[6 * a + c] += Jl[a] * Jp[c] + Jl[3 + a] * Jp[6 + c];
            for (int a = 0; a < 6; a++)
                for (int c = 0; c <= a; c++) h21[a * (a + 1) / 2 + c] += Jp[a] * Jp[c] + Jp[6 + a] * Jp[6 + c];
        }
        int status = lc == 1 ? COV_LMK_CONST : (lc == 2 ? COV_LMK_REDUCED : COV_LMK_ELIMINATED);
        double Hi[6] = {0, 0, 0, 0, 0, 0};
        if (status == COV_LMK_ELIMINATED && !(oe - ob >= 2 && cov_sym3_inverse(H, Hi))) { status = COV_LMK_SINGULAR; n = 0; }
        for (int e = 0; e < n; e++) {   // H_lp -> W = H_ll^-1 H_lp (zero for a landmark that is not eliminated)
            double* w18 = C.ent_w + (e0 + e) * COV_ENT_W;
            for (int c = 0; c < 6; c++) {
                double y[3] = {0.0, 0.0, 0.0};
                if (status == COV_LMK_ELIMINATED) cov_sym3_vec(Hi, w18[c], w18[6 + c], w18[12 + c], y);
                w18[c] = y[0]; w18[6 + c] = y[1]; w18[12 + c] = y[2];
            }
        }
        for (int q = 0; q < 6; q++) { C.hll[6 * (long long)l + q] = H[q]; C.hinv[6 * (long long)l + q] = Hi[q]; }
        C.status[l] = status;
        C.ent_n[l] = n;
    }
}

// The 6 x 6 pose block (a, b), a >= b, of S over the visual factors: sum_l [a == b] sum Jp^T Jp - W_a^T H_ll W_b.
__device__ __forceinline__ void cov_schur_body(const DevPtrs& P, const CovDev& C, const WinDev& W, int a, int b) {
    const int ca = a * W.dpf, cb = b * W.dpf;
    double acc[36];
#pragma unroll
    for (int q = 0; q < 36; q++) acc[q] = 0.0;
    for (int l = threadIdx.x; l < W.n_lmk; l += COV_SCHUR_THREADS) {
        const int n = C.ent_n[l];
        if (n == 0) continue;
        const long long e0 = P.lmk_ob[W.lmk_base + l] - W.obs_base;
        int ea = -1, eb = -1;
        for (int e = 0; e < n; e++) {
            const int col = C.ent_col[e0 + e];
            if (col == ca) ea = e;
            if (col == cb) eb = e;
        }
        if (ea < 0 || eb < 0) continue;
        if (a == b) {
            const double* h21 = C.ent_hpp + (e0 + ea) * COV_ENT_HPP;
#pragma unroll
            for (int i = 0; i < 6; i++)
#pragma unroll
                for (int j = 0; j < 6; j++) acc[6 * i + j] += i >= j ? h21[i * (i + 1) / 2 + j] : h21[j * (j + 1) / 2 + i];
        }
        if (C.status[l] != COV_LMK_ELIMINATED) continue;
        const double* Wa = C.ent_w + (e0 + ea) * COV_ENT_W;
        const double* Wb = C.ent_w + (e0 + eb) * COV_ENT_W;
        const double* H = C.hll + 6 * (long long)l;
        double HW[18];   // H_ll W_b
#pragma unroll
        for (int j = 0; j < 6; j++) {
            double y[3];
            cov_sym3_vec(H, Wb[j], Wb[6 + j], Wb[12 + j], y);
            HW[j] = y[0]; HW[6 + j] = y[1]; HW[12 + j] = y[2];
        }
#pragma unroll
        for (int i = 0; i < 6; i++)
#pragma unroll
            for (int j = 0; j < 6; j++) acc[6 * i + j] -= Wa[i] * HW[j] + Wa[6 + i] * HW[6 + j] + Wa[12 + i] * HW[12 + j];
    }
    __shared__ double sh[COV_SCHUR_THREADS * 36];
#pragma unroll
    for (int q = 0; q < 36; q++) sh[threadIdx.x * 36 + q] = acc[q];
    __syncthreads();
    for (int s = COV_SCHUR_THREADS / 2; s > 0; s >>= 1) {
        if ((int)threadIdx.x < s)
            for (int q = 0; q < 36; q++) sh[threadIdx.x * 36 + q] += sh[(threadIdx.x + s) * 36 + q];
        __syncthreads();
    }
    if (threadIdx.x < 36) {
        const int i = threadIdx.x / 6, j = threadIdx.x - 6 * i;
        if (a == b) C.S[(long long)(ca + i) * C.Np + ca + j] = 0.5 * (sh[6 * i + j] + sh[6 * j + i]);
        else {
            C.S[(long long)(ca + i) * C.Np + cb + j] = sh[6 * i + j];
            C.S[(long long)(cb + j) * C.Np + ca + i] = sh[6 * i + j];
        }
    }
}

__global__ __launch_bounds__(COV_SCHUR_THREADS) void k_cov_schur(DevPtrs P, CovDev C) {
    int a = 0, b;
    if (C.pair_tab) {   // band route: the pair comes from the table of in-band pairs
        a = C.pair_tab[2 * blockIdx.x]; b = C.pair_tab[2 * blockIdx.x + 1];
    } else {
        while ((a + 1) * (a + 2) / 2 <= (int)blockIdx.x) a++;
        b = (int)blockIdx.x - a * (a + 1) / 2;
    }
    const WinDev W = P.win[C.w];
    cov_schur_body(P, C, W, a, b);
}

// ---- the square-root assembly ----------------------------------------------------------------------------------------------------
// The same S and landmark blocks without the difference H_pp - W^T H_ll W: a landmark millimetres from a camera centre puts 1e12
// and more into H_pp beside entries of S of 1e10, and the plain form then loses S to rounding ("Near-camera landmarks").
// Per eliminated landmark J_l (2m x 3) = Q1 R; C_a = Q1^T J_p,a; its share of block (a, b) of S is the Gram sum
//   sum_r A_a[r]^T A_b[r],   A_a[r] = [row r is a's] J_p,a[r] - Q1[r] C_a      (the pose rows projected on the complement of range(J_l))
// over all 2m rows, and Sigma_ll = R^-1 (I + C Sigma_pp C^T) R^-T. Nothing is subtracted from anything large, S cannot come out
// indefinite, and Sigma_ll is positive semi-definite by construction. A landmark that is not eliminated has Q1 = 0, C = 0 and the
// same sum is its J_p^T J_p. k_cov_kept / k_cov_factors / k_cov_dense add their terms as on the plain route.
//
// k_cov_assemble_sqrt: k_cov_assemble's shape (a workgroup per tile, a thread per landmark). Q1 by Gram-Schmidt column after column
// with a second orthogonalisation pass (orthonormal to a few ulps while cond(J_l) eps < 1; R = chol(H_ll) would lose it with
// cond(H_ll)), in place on the landmark's rows of CovSqrtDev::q. Singular: fewer than two observations, or r_ii^2 <= 64 eps |column i|^2 —
// cov_sym3_inverse's pivot rule stated through R.
// What the square-root assembly keeps beside CovDev (a kernel argument of its own). On this route CovDev::hll holds R (upper: 00 01 02 11 12 22) and CovDev::ent_w the couplings C_a (3 x 6).
struct CovSqrtDev {
    double* jp;              // [n_obs][12] the two J_p rows of every observation
    double* q;               // [n_obs][6] the two rows of Q1 (zero for a landmark that is not eliminated)
    int* ent;                // [n_obs] entry of the observation's key-frame among its landmark's entries, -1: constant key-frame
    const int* kf_ptr;       // [n_free_kf + 1] CSR of the landmarks every free key-frame observes (cov_kf_lists.h) ...
    const int* kf_lmk;       // ... window landmark indices, ascending
};

template <int FACTOR>
__global__ __launch_bounds__(COV_THREADS) void k_cov_assemble_sqrt(DevPtrs P, CovDev C, CovSqrtDev Q1) {
    const WinDev W = P.win[C.w];
    const Tile T = P.tiles[W.tile_begin + blockIdx.x];
    for (int i = threadIdx.x; i < T.n_lmk; i += blockDim.x) {
        const int gl = tile_landmark(T, P.tile_lmk, i);
        const int l = gl - W.lmk_base;
        if (l < 0 || l >= W.n_lmk) continue;
        const int ob = P.lmk_ob[gl], oe = P.lmk_oe[gl];
        const long long e0 = ob - W.obs_base;
        const double* xl = P.xl + (long long)C.cur * P.xl_stride + 3 * (long long)gl;
        const double pw[3] = {P.lmk_p[3 * (long long)gl] + xl[0], P.lmk_p[3 * (long long)gl + 1] + xl[1], P.lmk_p[3 * (long long)gl + 2] + xl[2]};
        const int lc = P.lmk_const ? P.lmk_const[gl] : 0;
        int status = lc == 1 ? COV_LMK_CONST : (lc == 2 ? COV_LMK_REDUCED : COV_LMK_ELIMINATED);
        const bool elim = status == COV_LMK_ELIMINATED;
        double* Q = Q1.q + 6 * e0;         // row r of the landmark at Q[3 r]
        double* JP = Q1.jp + 12 * e0;      // row r at JP[6 r]
        int* EN = Q1.ent + e0;
        const int rows = 2 * (oe - ob);
        double cn[3] = {0.0, 0.0, 0.0};    // |column|^2 of J_l
        int n = 0;
        for (int o = ob; o < oe; o++) {
            double Jp[12], Jl[6];
            cov_obs_jacobians<FACTOR>(P, C, o, pw, Jp, Jl);
            for (int q = 0; q < 12; q++) JP[12 * (o - ob) + q] = Jp[q];
            for (int q = 0; q < 6; q++) Q[6 * (o - ob) + q] = elim ? Jl[q] : 0.0;
            for (int c = 0; c < 3; c++) cn[c] += Jl[c] * Jl[c] + Jl[3 + c] * Jl[3 + c];
            const int fi = P.kf_fidx[P.obs_kf[o]];
            if (fi < 0) { EN[o - ob] = -1; continue; }
            const int col = fi * W.dpf;
            int e = 0;
            while (e < n && C.ent_col[e0 + e] != col) e++;
            EN[o - ob] = e;
            if (e == n) {
                n++;
                C.ent_col[e0 + e] = col;
                double* c18 = C.ent_w + (e0 + e) * COV_ENT_W;
                for (int q = 0; q < COV_ENT_W; q++) c18[q] = 0.0;
            }
        }
        double R[6] = {0.0, 0.0, 0.0, 0.0, 0.0, 0.0};
        if (elim) {
            const double tol = 64.0 * 2.220446049250313e-16;
            bool ok = oe - ob >= 2;
            for (int j = 0; j < 3 && ok; j++) {
                for (int pass = 0; pass < 2; pass++)
                    for (int k = 0; k < j; k++) {
                        double s = 0.0;
                        for (int r = 0; r < rows; r++) s += Q[3 * r + k] * Q[3 * r + j];
                        for (int r = 0; r < rows; r++) Q[3 * r + j] -= s * Q[3 * r + k];
                        R[k == 0 ? j : 3 + j - 1] += s;   // (0, j) | (1, 2)
                    }
                double nn = 0.0;
                for (int r = 0; r < rows; r++) nn += Q[3 * r + j] * Q[3 * r + j];
                if (!(nn > tol * cn[j])) { ok = false; break; }
                const double rjj = sqrt(nn);
                R[j == 0 ? 0 : (j == 1 ? 3 : 5)] = rjj;
                for (int r = 0; r < rows; r++) Q[3 * r + j] /= rjj;
            }
            if (!ok) { status = COV_LMK_SINGULAR; n = 0; }
        }
        if (status == COV_LMK_ELIMINATED)   // C_a = Q1^T J_p,a, observation after observation
            for (int o = ob; o < oe; o++) {
                const int e = EN[o - ob];
                if (e < 0) continue;
                double* c18 = C.ent_w + (e0 + e) * COV_ENT_W;
                const double* q = Q + 6 * (o - ob);
                const double* jp = JP + 12 * (o - ob);
                for (int a = 0; a < 3; a++)
                    for (int c = 0; c < 6; c++) c18[6 * a + c] += q[a] * jp[c] + q[3 + a] * jp[6 + c];
            }
        for (int q = 0; q < 6; q++) C.hll[6 * (long long)l + q] = R[q];
        C.status[l] = status;
        C.ent_n[l] = n;
    }
}

// The 6 x 6 pose block (a, b), a >= b, of S over the visual factors in Gram form. The workgroup walks the landmarks key-frame a
// observes (CovSqrtDev::kf_ptr / kf_lmk, ascending landmark index: a fixed order) and looks for b among each landmark's entries; the partial
// sums and the tree are k_cov_schur's.
__global__ __launch_bounds__(COV_SCHUR_THREADS) void k_cov_schur_sqrt(DevPtrs P, CovDev C, CovSqrtDev Q1) {
    const WinDev W = P.win[C.w];
    int a = 0, b;
    if (C.pair_tab) {
        a = C.pair_tab[2 * blockIdx.x]; b = C.pair_tab[2 * blockIdx.x + 1];
    } else {
        while ((a + 1) * (a + 2) / 2 <= (int)blockIdx.x) a++;
        b = (int)blockIdx.x - a * (a + 1) / 2;
    }
    const int ca = a * W.dpf, cb = b * W.dpf;
    double acc[36];
#pragma unroll
    for (int q = 0; q < 36; q++) acc[q] = 0.0;
    const int it1 = Q1.kf_ptr[a + 1];
    for (int it = Q1.kf_ptr[a] + (int)threadIdx.x; it < it1; it += COV_SCHUR_THREADS) {
        const int l = Q1.kf_lmk[it];
        const int n = C.ent_n[l];
        if (n == 0) continue;
        const int ob = P.lmk_ob[W.lmk_base + l], oe = P.lmk_oe[W.lmk_base + l];
        const long long e0 = ob - W.obs_base;
        int ea = -1, eb = -1;
        for (int e = 0; e < n; e++) {
            const int col = C.ent_col[e0 + e];
            if (col == ca) ea = e;
            if (col == cb) eb = e;
        }
        if (ea < 0 || eb < 0) continue;
        double Ca[18], Cb[18];
#pragma unroll
        for (int q = 0; q < 18; q++) { Ca[q] = C.ent_w[(e0 + ea) * COV_ENT_W + q]; Cb[q] = C.ent_w[(e0 + eb) * COV_ENT_W + q]; }
        for (int o = ob; o < oe; o++) {
            const long long x = e0 + (o - ob);
            const int en = Q1.ent[x];
            const double* jp = Q1.jp + 12 * x;
            const double* q = Q1.q + 6 * x;
#pragma unroll
            for (int row = 0; row < 2; row++) {
                const double q0 = q[3 * row], q1 = q[3 * row + 1], q2 = q[3 * row + 2];
                double Aa[6], Ab[6];
#pragma unroll
                for (int i = 0; i < 6; i++) {
                    const double j = jp[6 * row + i];
                    Aa[i] = (en == ea ? j : 0.0) - (q0 * Ca[i] + q1 * Ca[6 + i] + q2 * Ca[12 + i]);
                    Ab[i] = (en == eb ? j : 0.0) - (q0 * Cb[i] + q1 * Cb[6 + i] + q2 * Cb[12 + i]);
                }
#pragma unroll
                for (int i = 0; i < 6; i++)
#pragma unroll
                    for (int j = 0; j < 6; j++) acc[6 * i + j] += Aa[i] * Ab[j];
            }
        }
    }
    __shared__ double sh[COV_SCHUR_THREADS * 36];
#pragma unroll
    for (int q = 0; q < 36; q++) sh[threadIdx.x * 36 + q] = acc[q];
    __syncthreads();
    for (int s = COV_SCHUR_THREADS / 2; s > 0; s >>= 1) {
        if ((int)threadIdx.x < s)
            for (int q = 0; q < 36; q++) sh[threadIdx.x * 36 + q] += sh[(threadIdx.x + s) * 36 + q];
        __syncthreads();
    }
    if (threadIdx.x < 36) {
        const int i = threadIdx.x / 6, j = threadIdx.x - 6 * i;
        if (a == b) C.S[(long long)(ca + i) * C.Np + ca + j] = 0.5 * (sh[6 * i + j] + sh[6 * j + i]);
        else {
            C.S[(long long)(ca + i) * C.Np + cb + j] = sh[6 * i + j];
            C.S[(long long)(cb + j) * C.Np + ca + i] = sh[6 * i + j];
        }
    }
}

// Landmarks kept in the reduced system: Jl^T Jl and Jl^T Jp of their observations (Jp^T Jp went through k_cov_schur).
template <int FACTOR>
__device__ __forceinline__ void cov_kept_body(const DevPtrs& P, const CovDev& C, const WinDev& W) {
    __shared__ double J[2 * 9];   // rows: [Jp 6 | Jl 3]
    __shared__ int col[9];
    const int t = threadIdx.x;
    for (int k = W.kept_begin; k < W.kept_end; k++) {
        const int o = P.kept_obs[3 * k], gl = P.kept_obs[3 * k + 1];
        if (P.obs_cam[o] < 0) continue;
        if (t == 0) {
            const double* xl = P.xl + (long long)C.cur * P.xl_stride + 3 * (long long)gl;
            const double pw[3] = {P.lmk_p[3 * (long long)gl] + xl[0], P.lmk_p[3 * (long long)gl + 1] + xl[1], P.lmk_p[3 * (long long)gl + 2] + xl[2]};
            double Jp[12], Jl[6];
            cov_obs_jacobians<FACTOR>(P, C, o, pw, Jp, Jl);
            const int fi = P.kf_fidx[P.obs_kf[o]], lr = P.lmk_red[gl];
            for (int q = 0; q < 2; q++) {
                for (int c = 0; c < 6; c++) J[9 * q + c] = Jp[6 * q + c];
                for (int c = 0; c < 3; c++) J[9 * q + 6 + c] = Jl[3 * q + c];
            }
            for (int c = 0; c < 6; c++) col[c] = fi >= 0 ? fi * W.dpf + c : -1;
            for (int c = 0; c < 3; c++) col[6 + c] = lr >= 0 ? lr + c : -1;
        }
        __syncthreads();
        for (int idx = t; idx < 81; idx += 64) {
            const int a = idx / 9, c = idx - 9 * a;
            if ((a < 6 && c < 6) || col[a] < 0 || col[c] < 0) continue;
            C.S[(long long)col[a] * C.Np + col[c]] += J[a] * J[c] + J[9 + a] * J[9 + c];
        }
        __syncthreads();
    }
}

template <int FACTOR>
__global__ __launch_bounds__(64) void k_cov_kept(DevPtrs P, CovDev C) {
    const WinDev W = P.win[C.w];
    cov_kept_body<FACTOR>(P, C, W);
}

// S[col a][col c] += sum_q J[q][a] J[q][c]: every (a, c) by one lane, factor after factor behind workgroup barriers
__device__ __forceinline__ void cov_accumulate(double* S, int Np, const double* J, int rows, int ncols, const int* col, int t, int nthr) {
    for (int idx = t; idx < ncols * ncols; idx += nthr) {
        const int a = idx / ncols, c = idx - a * ncols;
        if (col[a] < 0 || col[c] < 0) continue;
        double h = 0.0;
        for (int q = 0; q < rows; q++) h += J[q * ncols + a] * J[q * ncols + c];
        S[(long long)col[a] * Np + col[c]] += h;
    }
}

// ImuDev under a name of its own: imu_factor_body<CovImu, ..> is then an instantiation of its own, and the one k_marg_small calls
// keeps its single caller (with a second caller the compiler no longer specialises it on k_marg_small's constant arguments, and
// that kernel's code changes). For the same reason cov_factors_body takes the name as its template parameter IMU: every kernel
// that calls the body brings a name of its own (CovBatchImu in cov_batch_kernels.h), and each instantiation has one caller.
struct CovImu : ImuDev {};

template <class IMU>
__device__ __forceinline__ void cov_factors_body(const DevPtrs& P, const CovDev& C, const WinDev& W) {
    const int t = threadIdx.x;
    const double* xp = P.xp + (long long)C.cur * P.xp_stride;
    const double* xv = P.xv + (long long)C.cur * P.xv_stride;
    const double* xba = P.xba + (long long)C.cur * P.xv_stride;
    const double* xbg = P.xbg + (long long)C.cur * P.xv_stride;
    const double* xl = P.xl + (long long)C.cur * P.xl_stride;
    __shared__ double sJ[15 * 24];
    __shared__ int scol[24];
    // PosePriordx
    for (int k = W.prior_begin; k < W.prior_end; k++) {
        if (t == 0) {
            const PriorDev pr = P.priors[k];
            double T0[12], d6[6], r[6], J[36];
            for (int i = 0; i < 12; i++) T0[i] = P.kf_T0[12 * (long long)pr.kf + i];
            for (int i = 0; i < 6; i++) d6[i] = xp[6 * (long long)pr.kf + i];
            pose_prior_factor(T0, pr.T_prior, pr.inf, d6, r, J);
            const int fi = P.kf_fidx[pr.kf];
            for (int i = 0; i < 36; i++) sJ[i] = J[i];
            for (int a = 0; a < 6; a++) scol[a] = fi >= 0 ? fi * W.dpf + a : -1;
        }
        __syncthreads();
        cov_accumulate(C.S, C.Np, sJ, 6, 6, scol, t, 64);
        __syncthreads();
    }
    // IMUFactor + IMUBiasFactor (as k_marg_small evaluates them: lane 0 the un-whitened Jacobian, 24 lanes the whitening)
    for (int k = W.imu_begin; k < W.imu_end; k++) {
        const IMU& f = *static_cast<const IMU*>(P.imus + k);
        const int i = f.kf_i, j = f.kf_j;
        const int fi = P.kf_fidx[i], fj = P.kf_fidx[j];
        if (t == 0) {
            double r[9];
            for (int q = 0; q < 9 * 24; q++) sJ[q] = 0.0;
            imu_factor_body<IMU, false>(f, P.kf_T0 + 12 * (long long)i, P.kf_T0 + 12 * (long long)j, P.kf_vel + 3 * (long long)i, P.kf_vel + 3 * (long long)j,
                                        xp + 6 * (long long)i, xp + 6 * (long long)j, xv + 3 * (long long)i, xv + 3 * (long long)j, xba + 3 * (long long)i,
                                        xbg + 3 * (long long)i, r, sJ);
            for (int a = 0; a < 24; a++) scol[a] = W.dpf == 15 ? imu_col(a, fi, fj) : -1;
        }
        __syncthreads();
        if (t < 24) {   // J <- W J, W upper triangular (residuals.hpp:151-154)
            double u[9];
            for (int q = 0; q < 9; q++) u[q] = sJ[q * 24 + t];
            for (int q = 0; q < 9; q++) {
                double v = 0.0;
                for (int kk = q; kk < 9; kk++) v += f.W[9 * q + kk] * u[kk];
                sJ[q * 24 + t] = v;
            }
        }
        __syncthreads();
        cov_accumulate(C.S, C.Np, sJ, 9, 24, scol, t, 64);
        __syncthreads();
        if (t == 0) {   // bias random walk: r = s (b_j - b_i), columns ba_i | bg_i | ba_j | bg_j
            for (int q = 0; q < 72; q++) sJ[q] = 0.0;
            for (int a = 0; a < 3; a++) {
                sJ[a * 12 + a] = -f.sa; sJ[(3 + a) * 12 + 3 + a] = -f.sg; sJ[a * 12 + 6 + a] = f.sa; sJ[(3 + a) * 12 + 9 + a] = f.sg;
                const bool st = W.dpf == 15;
                scol[a] = st && fi >= 0 ? fi * 15 + 9 + a : -1; scol[3 + a] = st && fi >= 0 ? fi * 15 + 12 + a : -1;
                scol[6 + a] = st && fj >= 0 ? fj * 15 + 9 + a : -1; scol[9 + a] = st && fj >= 0 ? fj * 15 + 12 + a : -1;
            }
        }
        __syncthreads();
        cov_accumulate(C.S, C.Np, sJ, 6, 12, scol, t, 64);
        __syncthreads();
    }
    // the listed factors of the sparsified prior (the pose-to-landmark factors that ride the elimination are pseudo-observations)
    for (int q = W.spl_begin; q < W.spl_end; q++) {
        const SparseDev& f = P.sparse[P.sp_list[q]];
        __shared__ int s_rows;
        if (t == 0) {
            double r[15], J[225];
            for (int a = 0; a < 225; a++) J[a] = 0.0;
            const bool in = sparse_eval(P, W, f, xp, xv, xba, xbg, xl, nullptr, r, J);
            s_rows = in ? sparse_rows(f) : 0;
            for (int a = 0; a < 225; a++) sJ[a] = J[a];
            const int fi = f.kf >= 0 ? P.kf_fidx[f.kf] : -1;
            const int lr0 = sparse_lr0(P, W, f);
            const int lr1 = (f.lmk1 >= 0 && P.lmk_red) ? P.lmk_red[f.lmk1] : -1;
            for (int a = 0; a < 15; a++) scol[a] = sparse_col(f, a, fi, W.dpf, lr0, lr1);
        }
        __syncthreads();
        cov_accumulate(C.S, C.Np, sJ, s_rows, 15, scol, t, 64);
        __syncthreads();
    }
}

__global__ __launch_bounds__(64) void k_cov_factors(DevPtrs P, CovDev C) {
    const WinDev W = P.win[C.w];
    cov_factors_body<CovImu>(P, C, W);
}

// dense prior r0 + J dx: its J^T J (formed at upload) through the column map kind[n] | index[n] | col[n]
__device__ __forceinline__ void cov_dense_body(const DevPtrs& P, const CovDev& C, const WinDev& W) {
    const int n = W.dp_n;
    const long long idx = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (idx >= (long long)n * n) return;
    const int a = (int)(idx / n), c = (int)(idx - (long long)a * n);
    const int* col = P.dp_ints + W.dp_int_off + 2 * n;
    if (col[a] < 0 || col[c] < 0) return;
    const double* H = P.dp_data + W.dp_off + 2LL * W.dp_n_full * n;
    C.S[(long long)col[a] * C.Np + col[c]] += H[(long long)a * n + c];
}

__global__ void k_cov_dense(DevPtrs P, CovDev C) {
    const WinDev W = P.win[C.w];
    cov_dense_body(P, C, W);
}

// ---- the landmark blocks -----------------------------------------------------------------------------------------------------
// Sigma_ll = H_ll^-1 + sum_{e, f} W_e Sigma_pp(c_e, c_f) W_f^T over the (<= 64) observing key-frames of the landmark, all ordered
// pairs. One landmark per group of G lanes of a wave (G = 16: up to 4 observing key-frames per lane pass of 16 pairs, the usual
// window; G = 64: long tracks): lane q of the group takes the pairs q, q + G, ... in that order, the nine partial sums are combined
// by a butterfly inside the group — a fixed order, the same bits on every call. Sigma_pp (218 KB on the shipped VIO window) does
// not fit LDS and is read from global memory through the caches: a landmark with k observing key-frames reads k^2 blocks of
// 6 rows x 48 contiguous bytes; the matrix stays resident in L2 (4 MB per XCD), so HBM sees it once per XCD.
// SQRT (the square-root assembly): ent_w holds C and hll holds R; the same gather gives C Sigma_pp C^T, and the block is
// R^-1 (I + C Sigma_pp C^T) R^-T, its upper triangle computed and mirrored.
// A long track (CovDev::is_long) is skipped here: its gather is k_cov_lmk_long's (cov_long_kernels.h), its output formulas these.

// The landmark block of landmark l from the gathered sum acc = sum_{e, f} W_e Sigma_pp(c_e, c_f) W_f^T (square-root: C for W), by status
template <bool SQRT>
__device__ __forceinline__ void cov_lmk_write(const DevPtrs& P, const CovDev& C, const WinDev& W, int l, int status, const double* acc) {
    double* out = C.lout + 9 * (long long)l;
    if (SQRT && status == COV_LMK_ELIMINATED) {
        const double* R = C.hll + 6 * (long long)l;
        const double M[9] = {1.0 + acc[0], 0.5 * (acc[1] + acc[3]), 0.5 * (acc[2] + acc[6]), 0.0, 1.0 + acc[4], 0.5 * (acc[5] + acc[7]), 0.0, 0.0, 1.0 + acc[8]};
        double U[9] = {0, 0, 0, 0, 0, 0, 0, 0, 0};   // R^-1, upper
        U[0] = 1.0 / R[0]; U[4] = 1.0 / R[3]; U[8] = 1.0 / R[5];
        U[1] = -R[1] * U[4] / R[0];
        U[5] = -R[4] * U[8] / R[3];
        U[2] = -(R[1] * U[5] + R[2] * U[8]) / R[0];
        double Tm[9];   // U M, M symmetric
        for (int i = 0; i < 3; i++)
            for (int j = 0; j < 3; j++) {
                double v = 0.0;
                for (int k = i; k < 3; k++) v += U[3 * i + k] * (k <= j ? M[3 * k + j] : M[3 * j + k]);
                Tm[3 * i + j] = v;
            }
        for (int i = 0; i < 3; i++)
            for (int j = i; j < 3; j++) {
                double v = 0.0;
                for (int k = j; k < 3; k++) v += Tm[3 * i + k] * U[3 * j + k];
                out[3 * i + j] = v; out[3 * j + i] = v;
            }
    } else if (status == COV_LMK_ELIMINATED) {
        const double* Hi = C.hinv + 6 * (long long)l;
        const double s01 = 0.5 * (acc[1] + acc[3]), s02 = 0.5 * (acc[2] + acc[6]), s12 = 0.5 * (acc[5] + acc[7]);
        out[0] = Hi[0] + acc[0]; out[1] = Hi[1] + s01; out[2] = Hi[2] + s02;
        out[3] = out[1]; out[4] = Hi[3] + acc[4]; out[5] = Hi[4] + s12;
        out[6] = out[2]; out[7] = out[5]; out[8] = Hi[5] + acc[8];
    } else if (status == COV_LMK_REDUCED) {
        const int lr = P.lmk_red[W.lmk_base + l];
        for (int i = 0; i < 3; i++)
            for (int j = 0; j < 3; j++) out[3 * i + j] = C.Sig[(long long)(lr + i) * C.Np + lr + j];
    } else if (status == COV_LMK_SINGULAR) {
        for (int i = 0; i < 9; i++) out[i] = __builtin_nan("");
    } else {
        for (int i = 0; i < 9; i++) out[i] = 0.0;
    }
}

template <int G, bool SQRT = false>
__global__ __launch_bounds__(COV_THREADS) void k_cov_lmk(DevPtrs P, CovDev C) {
    const WinDev W = P.win[C.w];
    const int l = blockIdx.x * (COV_THREADS / G) + threadIdx.x / G;
    const int q = threadIdx.x % G;
    const bool have = l < W.n_lmk;
    const int status = have ? C.status[l] : COV_LMK_CONST;
    const bool lng = have && C.is_long && C.is_long[l];   // k_cov_lmk_long's
    const int n = (have && status == COV_LMK_ELIMINATED && !lng) ? C.ent_n[l] : 0;
    const long long e0 = have ? P.lmk_ob[W.lmk_base + l] - W.obs_base : 0;
    double acc[9];
#pragma unroll
    for (int i = 0; i < 9; i++) acc[i] = 0.0;
    for (int idx = q; idx < n * n; idx += G) {
        const int e = idx / n, f = idx - e * n;
        const double* We = C.ent_w + (e0 + e) * COV_ENT_W;
        const double* Wf = C.ent_w + (e0 + f) * COV_ENT_W;
        const double* Sg = C.Sig + (long long)C.ent_col[e0 + e] * C.Np + C.ent_col[e0 + f];
        double we[18], wf[18], T[18];
#pragma unroll
        for (int i = 0; i < 18; i++) { we[i] = We[i]; wf[i] = Wf[i]; T[i] = 0.0; }
#pragma unroll
        for (int k = 0; k < 6; k++) {
            double s[6];
#pragma unroll
            for (int j = 0; j < 6; j++) s[j] = Sg[(long long)k * C.Np + j];
#pragma unroll
            for (int i = 0; i < 3; i++)
#pragma unroll
                for (int j = 0; j < 6; j++) T[6 * i + j] += we[6 * i + k] * s[j];
        }
#pragma unroll
        for (int i = 0; i < 3; i++)
#pragma unroll
            for (int j = 0; j < 3; j++) {
                double v = 0.0;
#pragma unroll
                for (int k = 0; k < 6; k++) v += T[6 * i + k] * wf[6 * j + k];
                acc[3 * i + j] += v;
            }
    }
#pragma unroll
    for (int i = 0; i < 9; i++)
        for (int m = G / 2; m > 0; m >>= 1) acc[i] += __shfl_xor(acc[i], m, G);
    if (!have || lng || q != 0) return;
    cov_lmk_write<SQRT>(P, C, W, l, status, acc);
}

}  // namespace sadvio
