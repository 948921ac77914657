// cov_batch_kernels.h — marginal covariances of many windows per call (sadvio_ba_covariance_batch), device side.
//
// A "unit" is one window of the call (the items that name it share its assembly and its Sigma_pp). Every kernel below reads its
// window, delta buffer, N_p and the places of its work arrays from a table of CovUnit on the device, indexed by blockIdx.y (by
// blockIdx.x in k_cov_inv_lds); the grid's other dimension is sized for the largest unit of the launch and a workgroup beyond its
// own unit's extent leaves at once. The k_covb_* kernels are wrappers: each loads its unit's CovDev, applies that guard and calls the
// __device__ body that its k_cov_* counterpart in cov_kernels.h calls — one body per kernel, so the order in every sum
// (thread-strided partial sums, then the fixed tree) and the absence of floating-point atomics are those of the single call, and a
// unit's bits depend neither on the other units of the launch nor on its place among them. k_covb_assemble and k_covb_lmk alone
// are copies of k_cov_assemble's and k_cov_lmk's text behind the guard (cov_kernels.h says why): a change to one is made to the other.
// A unit with long tracks (handles created with SADVIO_CFG_LONG_TRACK_COVARIANCE | SADVIO_CFG_LONG_TRACK_BATCH): k_covb_long and
// k_covb_lmk_long, one workgroup per row of the group's work table (covb_long_plan.h), wrap cov_long_kernels.h's bodies the same way.
//
// k_cov_inv_lds is this file's own: Sigma_pp = S^-1 of one unit by ONE workgroup with the lower block triangle of S in LDS.
//   cap:      N_p <= COVB_CAP = 176 (11 block rows of 16; the shipped VIO window is 11 x 15 = 165)
//   layout:   66 tiles of 16 x 16, rows padded to 17 doubles (four row groups of a wave's ds_read_b64 land on four bank pairs) = 140.25 KiB,
//             + one work tile (the inverse of the current diagonal tile) + S's diagonal and the pivots' roots: 147 328 B of 160 KiB
//   steps:    1. S = L L^T, right-looking by block columns: the diagonal tile column after column with one barrier each and every
//                pivot tested as k_wfac_diag tests it (finite, above 1e-12 / N_p, not below 1024 N_p eps of its diagonal entry of S);
//                its inverse (16 lanes, one column each); the panel below as X L_KK^-T through that inverse; the trailing tiles
//             2. M = L^-1 in place: the diagonal tiles, then block column after block column from the right,
//                M_IJ = -(sum_K M_IK L_KJ) M_JJ
//             3. Sigma_pp = M^T M, tile (I, J) = sum_{K >= I} M_KI^T M_KJ from LDS straight into the unit's full symmetric slot
//   S is read from global memory once, Sigma_pp written once; nothing else leaves the CU between the steps.
//   tile products: plain FP64 VALU, 16 lanes per tile with a 4 x 4 register block each (the FP64 matrix cores have no rate
//   advantage on gfx950); 256 threads = 16 tile products in flight.
// A failed pivot sets the unit's flag; k_covb_lmk and the host's output stage skip such a unit.
// Part of the library's single translation unit; not a public header.
#pragma once
#include "cov_kernels.h"
#include "cov_long_kernels.h"

namespace sadvio {

constexpr int COVB_ROUTE_NONE = 0, COVB_ROUTE_LDS = 1, COVB_ROUTE_DENSE = 2;   // SADVIO_COV_ROUTE_*
constexpr int COVB_CAP = 176;
constexpr int COVB_LD = 17, COVB_TILE = 16 * COVB_LD;
constexpr int COVB_THREADS = 256, COVB_SLOTS = COVB_THREADS / 16;
static_assert(COVB_CAP % 16 == 0 && COVB_CAP / 16 - 1 <= COVB_SLOTS, "a block column's panel is one tile per slot");
static_assert(COVB_CAP <= COVB_THREADS, "one lane per column when the diagonal tiles are inverted");

__host__ __device__ constexpr int covb_lds_bytes(int nb) { return ((nb * (nb + 1) / 2 + 1) * COVB_TILE + 16 * nb + 16) * 8; }
static_assert(covb_lds_bytes(COVB_CAP / 16) <= 160 * 1024, "the LDS of one CU");

struct CovUnit {
    CovDev C;
    double* sig;     // C.Sig, writable
    int* bad;        // 1: a pivot of S is not safely positive
    int route;       // COVB_ROUTE_NONE | COVB_ROUTE_LDS
    int G;           // lanes per landmark of k_covb_lmk (16 | 64), 0: no landmark block asked of this unit
};

// ---- the wrappers: the unit's CovDev, the guard of a workgroup beyond the unit's extent, then cov_kernels.h's body ------------------
__global__ void k_covb_tables(DevPtrs P, const CovUnit* units, double* ptab) {
    const CovDev C = units[blockIdx.y].C;
    if (blockIdx.x == 0 && threadIdx.x == 0) *units[blockIdx.y].bad = 0;
    const WinDev W = P.win[C.w];
    cov_tables_body(P, C, W, ptab);
}

// (k_cov_assemble's text, which carries the comments)
template <int FACTOR>
__global__ __launch_bounds__(COV_THREADS) void k_covb_assemble(DevPtrs P, const CovUnit* units) {
    const CovDev C = units[blockIdx.y].C;
    const WinDev W = P.win[C.w];
    if ((int)blockIdx.x >= W.tile_end - W.tile_begin) return;
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
        for (int e = 0; e < n; e++) {
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

// The long tracks of the group's units (handles created with SADVIO_CFG_LONG_TRACK_COVARIANCE | SADVIO_CFG_LONG_TRACK_BATCH): the tile
// walk above never meets one. One workgroup of LONG_THREADS per row of the group's work table (covb_long_plan.h: unit inside the
// group | index on the long list), behind k_covb_assemble and in front of k_covb_schur: cov_long_kernels.h's plain body with the
// unit's CovDev, which fills the track's rows of the unit's tables and marks CovDev::is_long. A.max_kf is the table's (the LDS layout).
template <int FACTOR>
__global__ __launch_bounds__(LONG_THREADS) void k_covb_long(DevPtrs P, const CovUnit* units, const int* rows, LongArgs A) {
    extern __shared__ __attribute__((aligned(16))) char covb_long_smem[];
    const int* row = rows + 2 * (long long)blockIdx.x;
    const CovDev C = units[row[0]].C;
    cov_long_body<FACTOR, false>(P, C, CovSqrtDev{}, A, long_track(A, row[1]), covb_long_smem);
}

// ... and their landmark blocks, behind k_covb_lmk, which skips them: cov_long_kernels.h's body under k_covb_lmk's guard
__global__ __launch_bounds__(LONG_THREADS) void k_covb_lmk_long(DevPtrs P, const CovUnit* units, const int* rows, LongArgs A) {
    __shared__ double red[(LONG_THREADS / 64) * LONG_RED];
    const int* row = rows + 2 * (long long)blockIdx.x;
    const CovUnit U = units[row[0]];
    if (U.G == 0 || *U.bad) return;
    cov_lmk_long_body<false>(P, U.C, long_track(A, row[1]), red);
}

__global__ __launch_bounds__(COV_SCHUR_THREADS) void k_covb_schur(DevPtrs P, const CovUnit* units) {
    const CovDev C = units[blockIdx.y].C;
    const WinDev W = P.win[C.w];
    if (C.Np == 0 || (int)blockIdx.x >= W.n_free_kf * (W.n_free_kf + 1) / 2) return;
    int a = 0;   // (a unit of this call is never on the band route: no pair table)
    while ((a + 1) * (a + 2) / 2 <= (int)blockIdx.x) a++;
    cov_schur_body(P, C, W, a, (int)blockIdx.x - a * (a + 1) / 2);
}

template <int FACTOR>
__global__ __launch_bounds__(64) void k_covb_kept(DevPtrs P, const CovUnit* units) {
    const CovDev C = units[blockIdx.x].C;
    const WinDev W = P.win[C.w];
    if (C.Np == 0 || W.kept_end <= W.kept_begin) return;
    cov_kept_body<FACTOR>(P, C, W);
}

// ImuDev under a third name: an instantiation of imu_factor_body of this kernel's own (see CovImu in cov_kernels.h)
struct CovBatchImu : ImuDev {};

__global__ __launch_bounds__(64) void k_covb_factors(DevPtrs P, const CovUnit* units) {
    const CovDev C = units[blockIdx.x].C;
    if (C.Np == 0) return;
    const WinDev W = P.win[C.w];
    cov_factors_body<CovBatchImu>(P, C, W);
}

__global__ void k_covb_dense(DevPtrs P, const CovUnit* units) {
    const CovDev C = units[blockIdx.y].C;
    const WinDev W = P.win[C.w];
    if (C.Np == 0 || W.dp_n_full <= 0) return;
    cov_dense_body(P, C, W);
}

// ---- Sigma_pp = S^-1 inside one workgroup's LDS --------------------------------------------------------------------------------
__device__ __forceinline__ double* covb_tile(double* L, int I, int J) { return L + (I * (I + 1) / 2 + J) * COVB_TILE; }

// acc (4 x 4 at rows r0.., columns c0.. of a tile) += op(A) op(B): op(A)(i, k) = TA ? A[k][i] : A[i][k], op(B)(k, j) = TB ? B[j][k] : B[k][j]
template <bool TA, bool TB>
__device__ __forceinline__ void covb_mac(double (&acc)[16], const double* A, const double* B, int r0, int c0) {
#pragma unroll 4
    for (int k = 0; k < 16; k++) {
        double a[4], b[4];
#pragma unroll
        for (int q = 0; q < 4; q++) {
            a[q] = TA ? A[k * COVB_LD + r0 + q] : A[(r0 + q) * COVB_LD + k];
            b[q] = TB ? B[(c0 + q) * COVB_LD + k] : B[k * COVB_LD + c0 + q];
        }
#pragma unroll
        for (int i = 0; i < 4; i++)
#pragma unroll
            for (int j = 0; j < 4; j++) acc[4 * i + j] = __builtin_fma(a[i], b[j], acc[4 * i + j]);
    }
}

// column j of the inverse of the lower triangular tile T
__device__ __forceinline__ void covb_tri_inv_col(const double* T, int j, double (&m)[16]) {
#pragma unroll
    for (int i = 0; i < 16; i++) {
        double s = i == j ? 1.0 : 0.0;
#pragma unroll
        for (int k = 0; k < i; k++) s -= T[i * COVB_LD + k] * m[k];
        m[i] = i >= j ? s / T[i * COVB_LD + i] : 0.0;
    }
}

__global__ __launch_bounds__(COVB_THREADS) void k_cov_inv_lds(const CovUnit* units) {
    extern __shared__ __attribute__((aligned(16))) char covb_smem[];
    const CovUnit U = units[blockIdx.x];
    const int n = U.C.Np;
    if (U.route != COVB_ROUTE_LDS || n <= 0 || n > COVB_CAP) return;
    const int nb = (n + 15) >> 4, tid = threadIdx.x;
    double* L = (double*)covb_smem;
    double* Wt = L + nb * (nb + 1) / 2 * COVB_TILE;   // inverse of the current diagonal tile
    double* dg = Wt + COVB_TILE;                      // [16 nb] diagonal of S
    double* dd = dg + 16 * nb;                        // [16] roots of the current tile's pivots
    const double* S = U.C.S;
    const int ti = tid >> 4, tj = tid & 15;           // one element of a tile per thread
    const int slot = tid >> 4, r0 = 4 * ((tid & 15) >> 2), c0 = 4 * (tid & 3);   // one tile product per 16 lanes, 4 x 4 each
    // S -> LDS, lower block triangle; the columns past N_p continue the diagonal with ones
    for (int I = 0; I < nb; I++)
        for (int J = 0; J <= I; J++) {
            const int gi = 16 * I + ti, gj = 16 * J + tj;
            covb_tile(L, I, J)[ti * COVB_LD + tj] = (gi < n && gj < n) ? S[(long long)gi * n + gj] : (gi == gj ? 1.0 : 0.0);
        }
    for (int i = tid; i < 16 * nb; i += COVB_THREADS) dg[i] = i < n ? S[(long long)i * n + i] : 1.0;
    __syncthreads();
    const double tau = 1e-12 / n, safe_rel = 1024.0 * n * 2.220446049250313e-16;
    // 1. S = L L^T
    for (int K = 0; K < nb; K++) {
        double* T = covb_tile(L, K, K);
        bool fail = false;
        for (int c = 0; c < 16; c++) {   // every thread reads the same pivot: the test's outcome is uniform over the workgroup
            const double p = T[c * COVB_LD + c];
            if (16 * K + c < n && !(p > tau && p >= safe_rel * dg[16 * K + c] && p < 1e300)) { fail = true; break; }
            const double inv = 1.0 / p;
            if (tj > c && ti >= tj) T[ti * COVB_LD + tj] -= T[ti * COVB_LD + c] * T[tj * COVB_LD + c] * inv;
            if (tid == 0) dd[c] = sqrt(p);
            __syncthreads();
        }
        if (fail) {
            if (tid == 0) *U.bad = 1;
            return;
        }
        {
            const double v = T[ti * COVB_LD + tj];
            T[ti * COVB_LD + tj] = tj < ti ? v / dd[tj] : (ti == tj ? dd[ti] : 0.0);
        }
        __syncthreads();
        if (K + 1 == nb) break;
        if (tid < 16) {
            double m[16];
            covb_tri_inv_col(T, tid, m);
#pragma unroll
            for (int i = 0; i < 16; i++) Wt[i * COVB_LD + tid] = m[i];
        }
        __syncthreads();
        {   // the panel: X <- X L_KK^-T
            const int I = K + 1 + slot;
            double acc[16];
#pragma unroll
            for (int q = 0; q < 16; q++) acc[q] = 0.0;
            if (I < nb) covb_mac<false, true>(acc, covb_tile(L, I, K), Wt, r0, c0);
            __syncthreads();
            if (I < nb) {
                double* X = covb_tile(L, I, K);
#pragma unroll
                for (int a = 0; a < 4; a++)
#pragma unroll
                    for (int b = 0; b < 4; b++) X[(r0 + a) * COVB_LD + c0 + b] = acc[4 * a + b];
            }
            __syncthreads();
        }
        const int m = nb - K - 1;
        for (int t = slot; t < m * (m + 1) / 2; t += COVB_SLOTS) {   // trailing tiles (I, J), K < J <= I
            int a = 0;
            while ((a + 1) * (a + 2) / 2 <= t) a++;
            const int I = K + 1 + a, J = K + 1 + t - a * (a + 1) / 2;
            double acc[16];
#pragma unroll
            for (int q = 0; q < 16; q++) acc[q] = 0.0;
            covb_mac<false, true>(acc, covb_tile(L, I, K), covb_tile(L, J, K), r0, c0);
            double* Cm = covb_tile(L, I, J);
#pragma unroll
            for (int a2 = 0; a2 < 4; a2++)
#pragma unroll
                for (int b = 0; b < 4; b++) Cm[(r0 + a2) * COVB_LD + c0 + b] -= acc[4 * a2 + b];
        }
        __syncthreads();
    }
    // 2. M = L^-1 in place. The diagonal tiles first: one lane per column of the matrix
    {
        double m[16];
        const bool act = tid < 16 * nb;
        if (act) covb_tri_inv_col(covb_tile(L, tid >> 4, tid >> 4), tid & 15, m);
        __syncthreads();
        if (act) {
            double* T = covb_tile(L, tid >> 4, tid >> 4);
#pragma unroll
            for (int i = 0; i < 16; i++) T[i * COVB_LD + (tid & 15)] = m[i];
        }
        __syncthreads();
    }
    for (int J = nb - 2; J >= 0; J--) {   // M_IJ = -(sum_{K = J+1..I} M_IK L_KJ) M_JJ, I > J
        const int I = J + 1 + slot;
        double acc[16];
#pragma unroll
        for (int q = 0; q < 16; q++) acc[q] = 0.0;
        if (I < nb)
            for (int K = J + 1; K <= I; K++) covb_mac<false, false>(acc, covb_tile(L, I, K), covb_tile(L, K, J), r0, c0);
        __syncthreads();
        if (I < nb) {
            double* X = covb_tile(L, I, J);
#pragma unroll
            for (int a = 0; a < 4; a++)
#pragma unroll
                for (int b = 0; b < 4; b++) { X[(r0 + a) * COVB_LD + c0 + b] = acc[4 * a + b]; acc[4 * a + b] = 0.0; }
        }
        __syncthreads();
        if (I < nb) covb_mac<false, false>(acc, covb_tile(L, I, J), covb_tile(L, J, J), r0, c0);
        __syncthreads();
        if (I < nb) {
            double* X = covb_tile(L, I, J);
#pragma unroll
            for (int a = 0; a < 4; a++)
#pragma unroll
                for (int b = 0; b < 4; b++) X[(r0 + a) * COVB_LD + c0 + b] = -acc[4 * a + b];
        }
        __syncthreads();
    }
    // 3. Sigma_pp = M^T M, tile (I, J) = sum_{K >= I} M_KI^T M_KJ, written to both triangles. (i, j) and (j, i) of a diagonal tile
    // are the same products in the same order: the block is symmetric to the bit.
    for (int t = slot; t < nb * (nb + 1) / 2; t += COVB_SLOTS) {
        int I = 0;
        while ((I + 1) * (I + 2) / 2 <= t) I++;
        const int J = t - I * (I + 1) / 2;
        double acc[16];
#pragma unroll
        for (int q = 0; q < 16; q++) acc[q] = 0.0;
        for (int K = I; K < nb; K++) covb_mac<true, false>(acc, covb_tile(L, K, I), covb_tile(L, K, J), r0, c0);
#pragma unroll
        for (int a = 0; a < 4; a++)
#pragma unroll
            for (int b = 0; b < 4; b++) {
                const int gi = 16 * I + r0 + a, gj = 16 * J + c0 + b;
                if (gi >= n || gj >= n) continue;
                U.sig[(long long)gi * n + gj] = acc[4 * a + b];
                if (I != J) U.sig[(long long)gj * n + gi] = acc[4 * a + b];
            }
    }
}

// ---- the landmark blocks ---------------------------------------------------------------------------------------------------------
template <int G>
__global__ __launch_bounds__(COV_THREADS) void k_covb_lmk(DevPtrs P, const CovUnit* units) {
    const CovUnit U = units[blockIdx.y];
    if (U.G != G || *U.bad) return;
    const CovDev C = U.C;
    const WinDev W = P.win[C.w];
    const int l = blockIdx.x * (COV_THREADS / G) + threadIdx.x / G;
    const int q = threadIdx.x % G;
    const bool have = l < W.n_lmk;
    const int status = have ? C.status[l] : COV_LMK_CONST;
    const bool lng = have && C.is_long && C.is_long[l];   // k_covb_lmk_long's
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
    double* out = C.lout + 9 * (long long)l;
    if (status == COV_LMK_ELIMINATED) {
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

}  // namespace sadvio
