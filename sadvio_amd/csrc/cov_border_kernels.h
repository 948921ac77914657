// cov_border_kernels.h — the BORDER route of sadvio_ba_covariance: a long window whose S is block-banded but for the couplings of a
// few key-frames (loop closures). cov_border_plan.h picks those key-frames; with the reduced columns ordered [core | border]
//     S = [ B  C ]     B: n_b x n_b, block-banded (bw = (hb' + 1) * dpf)
//         [ C^T D ]    D: m x m dense, m <= COV_BORDER_MAXM
// and B = L L^T (k_cov_band_chol), the band of B^-1 (k_cov_band_sel), W = B^-1 C, T = D - C^T W = R R^T:
//     Sigma_DD = T^-1      Sigma_BD = -W T^-1 = -Z      Sigma_BB(i, j) = B^-1(i, j) + (Z W^T)(i, j)
// The pivots of B followed by those of T are the pivots of S in this order, so the band route's three pivot tests apply to both and
// both write the same flag. Kernels, in launch order (the two band sweeps between the first and the second are cov_band_kernels.h's,
// run as they are on the compacted image of B):
//   k_cov_border_split   gathers from the naturally ordered S the lower band of B into a compacted n_b x n_b image, C (column after
//                        column) and D.
//   k_cov_border_solve   W = B^-1 C by substitution with L's band: k_cov_band_cols' loop for a general right-hand side. One workgroup
//                        per border key-frame, one group of 16 lanes per column of C, row after row, forward then backward.
//   k_cov_border_schur   one workgroup: T (one wave per entry, a butterfly over its 64 lanes), its Cholesky factor in LDS with every
//                        pivot tested, R^-1, T^-1 = R^-T R^-1 (lower triangle and mirror), Z = W T^-1.
//   k_cov_border_apply   one workgroup per core key-frame: Sigma_BB's in-band blocks of its block row, Sigma_BD and Sigma_DB of its rows;
//                        one more workgroup writes Sigma_DD. Everything goes to the NATURAL positions of Sigma [N_p][N_p], so
//                        k_cov_lmk*, and the pickers read as on the band route. Both triangles come from one computed value.
//   k_cov_border_gather  the blocks asked for, packed; a pair of two core key-frames outside the core band is k_cov_band_cols' column of
//                        B^-1 plus the same Z W^T term (the block and its transpose from one formula: equal to the bit).
// All FP64 on the VALU (cov_band_kernels.h says why); every sum in a fixed order; no floating-point atomics; no flag or wait between
// workgroups. LDS: k_cov_border_schur holds T and R^-1, 2 m^2 doubles (147 KB at m = 96), alone on its CU.
// Part of the library's single translation unit; not a public header.
#pragma once
#include "cov_band_kernels.h"
#include "cov_border_plan.h"

namespace sadvio {

constexpr int COVBORDER_ZC = 32;   // columns of Z a lane of k_cov_border_schur holds at a time

struct CovBorder {
    int n, nc, m;            // N_p | n_b: columns of the core | columns of the border
    int bw, M, dpf;          // of the core's band: (hb' + 1) * dpf | bw + NB (the row length of Lb)
    double tau, safe_rel;    // pivot tests, as CovBand's (safe_rel of N_p)
    const int* perm;         // [n] natural column of position p of [core | border]
    const double* S;         // [n][n] natural
    double* Sig;             // [n][n] natural
    double* Sb;              // [nc][nc] compacted B, lower band
    double* Sigc;            // [nc][nc] compacted band of B^-1 (k_cov_band_sel)
    const double* Lb;        // [nc][M] L's band (k_cov_band_chol)
    double* Ct;              // [m][nc] C, column after column
    double* Dm;              // [m][m]
    double* W;               // [m][nc]
    double* Z;               // [m][nc]
    double* Tinv;            // [m][m]
    int* flag;               // the route's pivot flag
};

inline size_t covborder_lds_bytes(int m) { return sizeof(double) * 2 * (size_t)m * m; }

__global__ __launch_bounds__(COVBAND_THREADS) void k_cov_border_split(CovBorder B) {
    const long long nband = (long long)B.nc * B.bw, nC = (long long)B.m * B.nc, nD = (long long)B.m * B.m;
    const long long idx = (long long)blockIdx.x * COVBAND_THREADS + threadIdx.x;
    const int n = B.n, nc = B.nc;
    if (idx < nband) {
        const int i = (int)(idx / B.bw), j = i - (int)(idx - (long long)i * B.bw);
        if (j >= 0) B.Sb[(long long)i * nc + j] = B.S[(long long)B.perm[i] * n + B.perm[j]];
    } else if (idx < nband + nC) {
        const long long e = idx - nband;
        const int c = (int)(e / nc), i = (int)(e - (long long)c * nc);
        B.Ct[e] = B.S[(long long)B.perm[i] * n + B.perm[nc + c]];
    } else if (idx < nband + nC + nD) {
        const long long e = idx - nband - nC;
        const int a = (int)(e / B.m), b = (int)(e - (long long)a * B.m);
        B.Dm[e] = B.S[(long long)B.perm[nc + a] * n + B.perm[nc + b]];
    }
}

// W[c][:] = B^-1 C[:, c] for the dpf columns c of border key-frame blockIdx.x: L Y = C, L^T W = Y with L's band. Group g of 16 lanes
// takes column blockIdx.x * dpf + g; lane q of the group takes the terms q, q + 16, ... of a row's sum in that order and the 16 partial
// sums are combined by a butterfly, as in k_cov_band_cols. The last M values of the solved vector sit in LDS; a row's entries of L and
// its right-hand side are loaded one row ahead of their use.
__global__ __launch_bounds__(COVBAND_THREADS) void k_cov_border_solve(CovBorder B) {
    const int n = B.nc, M = B.M, bw = B.bw, dpf = B.dpf, t = threadIdx.x;
    if (*B.flag != 0) return;
    __shared__ double win[COVBAND_THREADS / COVBAND_GROUP][COVBAND_MAXW];
    const int g = t / COVBAND_GROUP, q = t % COVBAND_GROUP;
    const bool act = g < dpf;
    const size_t c = (size_t)blockIdx.x * dpf + (act ? g : 0);
    const double* Cg = B.Ct + c * n;
    double* Wg = B.W + c * n;
    double* wg = win[g];
    double lv[COVBAND_LV], ld = 0.0, rh = 0.0;
    auto fetch_f = [&](int i) {
#pragma unroll
        for (int u = 0; u < COVBAND_LV; u++) {
            const int k = i - 1 - q - COVBAND_GROUP * u;
            lv[u] = (i < n && k >= 0 && i - k < bw) ? B.Lb[(long long)i * M + (i - k)] : 0.0;
        }
        ld = i < n ? B.Lb[(long long)i * M] : 1.0;
        rh = i < n ? Cg[i] : 0.0;
    };
    fetch_f(0);
    for (int i = 0; i < n; i++) {
        double s = 0.0;
#pragma unroll
        for (int u = 0; u < COVBAND_LV; u++) {
            const int k = i - 1 - q - COVBAND_GROUP * u;
            if (k >= 0 && i - k < bw) s += lv[u] * wg[k % M];
        }
        const double d = ld, r = rh;
        fetch_f(i + 1);
#pragma unroll
        for (int m = COVBAND_GROUP / 2; m > 0; m >>= 1) s += __shfl_xor(s, m, COVBAND_GROUP);
        const double y = (r - s) / d;
        if (q == 0 && act) { wg[i % M] = y; Wg[i] = y; }
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
            const double x = (Wg[i] - s) / d;
            wg[i % M] = x; Wg[i] = x;
        }
        __syncthreads();
    }
}

__global__ __launch_bounds__(COVBAND_THREADS) void k_cov_border_schur(CovBorder B) {
    extern __shared__ double cbr_lds[];
    const int nc = B.nc, m = B.m, t = threadIdx.x;
    if (*B.flag != 0) return;            // (uniform) B's factor is not usable
    double* T = cbr_lds;                 // T, then R (lower), then T^-1
    double* U = T + (size_t)m * m;       // R^-1 (lower)
    __shared__ int s_fail;
    if (t == 0) s_fail = 0;
    // T = D - C^T W, lower triangle and mirror: wave after wave takes an entry, lane q the rows q, q + 64, ...
    {
        const int wv = t / 64, q = t % 64;
        for (int e = wv; e < m * m; e += COVBAND_THREADS / 64) {
            const int a = e / m, b = e - a * m;
            if (b > a) continue;
            const double* Ca = B.Ct + (size_t)a * nc;
            const double* Wb = B.W + (size_t)b * nc;
            double s = 0.0;
            for (int i = q; i < nc; i += 64) s += Ca[i] * Wb[i];
#pragma unroll
            for (int k = 32; k > 0; k >>= 1) s += __shfl_xor(s, k, 64);
            if (q == 0) { const double v = B.Dm[e] - s; T[a * m + b] = v; T[b * m + a] = v; }
        }
    }
    __syncthreads();
    // R R^T = T, right-looking, column after column; every pivot tested as k_cov_band_chol tests it
    for (int k = 0; k < m; k++) {
        if (t == 0) {
            const double piv = T[k * m + k], a0 = B.Dm[k * m + k];
            if (!(piv > B.tau && piv >= B.safe_rel * a0 && piv < 1e300)) s_fail = 1;
            T[k * m + k] = sqrt(piv);
        }
        __syncthreads();
        if (s_fail) break;
        const double inv = 1.0 / T[k * m + k];
        for (int i = k + 1 + t; i < m; i += COVBAND_THREADS) T[i * m + k] *= inv;
        __syncthreads();
        const int r = m - k - 1;
        for (int idx = t; idx < r * r; idx += COVBAND_THREADS) {
            const int ii = idx / r, jj = idx - ii * r;
            if (jj > ii) continue;
            T[(k + 1 + ii) * m + k + 1 + jj] -= T[(k + 1 + ii) * m + k] * T[(k + 1 + jj) * m + k];
        }
        __syncthreads();
    }
    if (s_fail) { if (t == 0) *B.flag = 1; return; }
    // U = R^-1, one lane per column
    for (int j = t; j < m; j += COVBAND_THREADS) {
        for (int i = 0; i < j; i++) U[i * m + j] = 0.0;
        U[j * m + j] = 1.0 / T[j * m + j];
        for (int i = j + 1; i < m; i++) {
            double v = 0.0;
            for (int k = j; k < i; k++) v += T[i * m + k] * U[k * m + j];
            U[i * m + j] = -v / T[i * m + i];
        }
    }
    __syncthreads();
    // T^-1 = R^-T R^-1, lower triangle and mirror
    for (int e = t; e < m * m; e += COVBAND_THREADS) {
        const int a = e / m, b = e - a * m;
        if (b > a) continue;
        double v = 0.0;
        for (int k = a; k < m; k++) v += U[k * m + a] * U[k * m + b];
        T[a * m + b] = v; T[b * m + a] = v;
        B.Tinv[a * m + b] = v; B.Tinv[b * m + a] = v;
    }
    __syncthreads();
    // Z[c][i] = sum_b W[b][i] T^-1[b][c], b ascending: one lane per row i, COVBORDER_ZC columns c at a time in registers
    for (int i = t; i < nc; i += COVBAND_THREADS)
        for (int c0 = 0; c0 < m; c0 += COVBORDER_ZC) {
            double acc[COVBORDER_ZC];
#pragma unroll
            for (int u = 0; u < COVBORDER_ZC; u++) acc[u] = 0.0;
            for (int b = 0; b < m; b++) {
                const double w = B.W[(size_t)b * nc + i];
#pragma unroll
                for (int u = 0; u < COVBORDER_ZC; u++)
                    if (c0 + u < m) acc[u] += w * T[b * m + c0 + u];
            }
#pragma unroll
            for (int u = 0; u < COVBORDER_ZC; u++)
                if (c0 + u < m) B.Z[(size_t)(c0 + u) * nc + i] = acc[u];
        }
}

// (Z W^T)(i, j) = sum_c Z[c][i] W[c][j], c ascending
__device__ __forceinline__ double covborder_zw(const CovBorder& B, int i, int j) {
    double s = 0.0;
    for (int c = 0; c < B.m; c++) s += B.Z[(size_t)c * B.nc + i] * B.W[(size_t)c * B.nc + j];
    return s;
}

// hb: hb' of the core. Workgroup a < nc / dpf: block row a of the core; workgroup nc / dpf: Sigma_DD.
__global__ __launch_bounds__(COVBAND_THREADS) void k_cov_border_apply(CovBorder B, int hb) {
    const int n = B.n, nc = B.nc, m = B.m, dpf = B.dpf, t = threadIdx.x, a = blockIdx.x;
    if (*B.flag != 0) return;
    if (a == nc / dpf) {
        for (int e = t; e < m * m; e += COVBAND_THREADS) {
            const int r = e / m, c = e - r * m;
            B.Sig[(long long)B.perm[nc + r] * n + B.perm[nc + c]] = B.Tinv[e];
        }
        return;
    }
    const int b0 = max(0, a - hb), bs = dpf * dpf;
    for (int e = t; e < (a - b0 + 1) * bs; e += COVBAND_THREADS) {
        const int b = b0 + e / bs, r = e - (b - b0) * bs, ii = r / dpf, jj = r - ii * dpf;
        const int i = a * dpf + ii, j = b * dpf + jj;
        if (j > i) continue;
        const double v = B.Sigc[(long long)i * nc + j] + covborder_zw(B, i, j);
        const long long pi = B.perm[i], pj = B.perm[j];
        B.Sig[pi * n + pj] = v; B.Sig[pj * n + pi] = v;
    }
    for (int e = t; e < m * dpf; e += COVBAND_THREADS) {
        const int c = e / dpf, i = a * dpf + (e - c * dpf);
        const double v = -B.Z[(size_t)c * nc + i];
        const long long pi = B.perm[i], pc = B.perm[nc + c];
        B.Sig[pi * n + pc] = v; B.Sig[pc * n + pi] = v;
    }
}

// Block e of the call's answer, as k_cov_band_gather; tab[4 e ..]: kind | r0 | c0 | x
//   0 zeros   1 Sigma[r0 + i][c0 + j], natural   2 X[x][j][r0 + i] + (Z W^T)(r0 + i, c0 + j), compacted core rows and columns,
//   3 the transpose of kind 2's block
__global__ __launch_bounds__(COVBAND_THREADS) void k_cov_border_gather(CovBorder B, const int* __restrict__ tab, const double* __restrict__ X, double* __restrict__ out) {
    const int dpf = B.dpf, n = B.n, nc = B.nc, t = threadIdx.x;
    if (t >= dpf * dpf) return;
    if (*B.flag != 0) return;
    const int kind = tab[4 * blockIdx.x], r0 = tab[4 * blockIdx.x + 1], c0 = tab[4 * blockIdx.x + 2], x = tab[4 * blockIdx.x + 3];
    int i = t / dpf, j = t - i * dpf;
    double v = 0.0;
    if (kind == COVBAND_G_SIG) v = B.Sig[(long long)(r0 + i) * n + c0 + j];
    else if (kind == COVBAND_G_COL || kind == COVBAND_G_COLT) {
        if (kind == COVBAND_G_COLT) { const int s = i; i = j; j = s; }
        v = X[((size_t)x * dpf + j) * nc + r0 + i] + covborder_zw(B, r0 + i, c0 + j);
    }
    out[(size_t)blockIdx.x * dpf * dpf + t] = v;
}

}  // namespace sadvio
