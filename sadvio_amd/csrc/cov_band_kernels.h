// cov_band_kernels.h — the band route of sadvio_ba_covariance: the blocks of Sigma_pp = S^-1 inside the band of a block-banded S
// (selected inversion), without a dense factor, a dense inverse or an N_p^2 transfer. All of it FP64.
//
// S of a long window without a dense prior, kept landmarks or lines has no non-zero at |i - j| >= bw = (hb + 1) * dpf
// (solve_driver.h: window_bandwidth). Every block the call returns, and every block of Sigma_pp that k_cov_lmk reads, lies at
// |i - j| < bw as well. Kernels, in launch order:
//   k_cov_band_chol   one workgroup: S = L L^T, right-looking in block columns of NB (6 for dpf 6, 5 for dpf 15, as k_band_solve).
//                     The live rows [c0, c0 + M), M = bw + NB, sit in LDS as a circular M x M image (element (i, j) at
//                     [(i % M) * M + j % M], lower triangle); per block column: one lane factors and inverts the NB x NB pivot
//                     block in registers, every pivot tested as factor_unpivoted tests it (finite and positive, above tau, above
//                     safe_rel of its entry of S); one lane per panel entry forms L_Jj = A_Jj L_jj^-T; the trailing update over the
//                     (bw - 1)^2 / 2 entries below; the NB rows that enter the window are loaded. L goes to global memory as
//                     Lb[i][i - j] (N_p x M doubles), the inverse pivot blocks beside it. A failed test sets the flag and ends the
//                     sweep; the host reads the flag behind the call's one wait.
//   k_cov_band_sel    one workgroup: the Takahashi recursion over the block columns j = K - 1 .. 0, J the (up to bw - 1) rows below:
//                       T = L_Jj L_jj^-1,  Sigma_Jj = -Sigma_JJ T,  Sigma_jj = L_jj^-T L_jj^-1 - Sigma_Jj^T T
//                     (the last is (L_jj^-T - Sigma_Jj^T L_Jj) L_jj^-1 multiplied out; its lower triangle is computed and mirrored, so
//                     a diagonal block is symmetric to the bit). Sigma_JJ is the same circular M x M image, both triangles. Both
//                     triangles of the band go to Sigma (dense-addressed, [i * N_p + j]); nothing else of Sigma is written.
//   k_cov_band_cols   Sigma(:, b) for a key-frame b some pair block outside the band names: S X = E_b by substitution with L's band,
//                     one workgroup per distinct b, one group of 16 lanes per right-hand side, row after row.
//   k_cov_band_gather the blocks asked for, packed: one workgroup per block.
// Every sum is taken in a fixed order (a lane's loop, then a butterfly inside a group of 16 lanes); no floating-point atomics; no
// flag or wait between workgroups: the chains live inside one workgroup each. The panel products run on the VALU: at bw = 30 a block
// column is 29 x 29 x 6 multiply-adds spread over 256 lanes between workgroup barriers, which the barriers dominate; FP64 MFMA has
// no rate advantage on this chip and would add a layout shuffle per step.
// LIMIT: the M x M image and three M x NB panels must fit LDS: bw + NB <= COVBAND_MAXW = 128 (dpf 6: hb <= 19; dpf 15: hb <= 7).
// Part of the library's single translation unit; not a public header.
#pragma once
#include "cov_kernels.h"

namespace sadvio {

constexpr int COVBAND_THREADS = 256;
constexpr int COVBAND_MAXW = 128;
constexpr int COVBAND_GROUP = 16;                      // lanes per right-hand side of k_cov_band_cols
constexpr int COVBAND_LV = COVBAND_MAXW / COVBAND_GROUP;

struct CovBand {
    int n, bw, M;            // N_p | rows below a column that can be non-zero, itself included | bw + NB
    int dpf;
    double tau, safe_rel;    // pivot tests: piv > tau, piv >= safe_rel * S[g][g]
    const double* S;         // [n][n]
    double* Sig;             // [n][n]
    double* Lb;              // [n][M]: L[i][j] at i * M + (i - j)
    double* Linv;            // [n / NB][NB * NB] inverse pivot blocks, lower, row-major
    int* flag;               // != 0: a pivot failed its test
};

inline size_t covband_lds_bytes(int M, int nb) { return sizeof(double) * ((size_t)M * M + 3 * (size_t)M * nb + 2 * (size_t)nb * nb); }

template <int NB>
__global__ __launch_bounds__(COVBAND_THREADS) void k_cov_band_chol(CovBand B) {
    extern __shared__ double cb_lds[];
    const int n = B.n, M = B.M, bw = B.bw, t = threadIdx.x;
    double* A = cb_lds;                  // circular image of the live rows, lower triangle
    double* Pn = A + (size_t)M * M;      // L_Jj, [row - r0][NB]
    double* D = Pn + 3 * (size_t)M * NB; // L_jj^-1, lower, row-major
    __shared__ int s_fail;
    if (t == 0) s_fail = 0;
    // rows 0 .. min(M, n) - 1: the band from S, zero beyond it (the panel of a block column reaches NB - 1 entries past the band)
    for (int idx = t; idx < M * M; idx += COVBAND_THREADS) {
        const int i = idx / M, jj = idx - i * M, j = i - jj;
        if (i < n && j >= 0) A[i * M + j] = jj < bw ? B.S[(long long)i * n + j] : 0.0;
    }
    __syncthreads();
    for (int c0 = 0; c0 < n; c0 += NB) {
        const int r0 = c0 + NB, r1 = min(n, c0 + NB + bw - 1), r = r1 - r0;
        if (t == 0) {
            double L[NB][NB], I[NB][NB];
#pragma unroll
            for (int i = 0; i < NB; i++)
#pragma unroll
                for (int k = 0; k <= i; k++) L[i][k] = A[((c0 + i) % M) * M + (c0 + k) % M];
            bool ok = true;
#pragma unroll
            for (int k = 0; k < NB; k++) {
                double piv = L[k][k];
#pragma unroll
                for (int m = 0; m < k; m++) piv -= L[k][m] * L[k][m];
                const double a0 = B.S[(long long)(c0 + k) * n + c0 + k];
                if (!(piv > B.tau && piv >= B.safe_rel * a0 && piv < 1e300)) ok = false;
                const double lkk = sqrt(piv), inv = 1.0 / lkk;
                L[k][k] = lkk; I[k][k] = inv;
#pragma unroll
                for (int i = k + 1; i < NB; i++) {
                    double v = L[i][k];
#pragma unroll
                    for (int m = 0; m < k; m++) v -= L[i][m] * L[k][m];
                    L[i][k] = v * inv;
                }
            }
#pragma unroll
            for (int j = 0; j < NB; j++)      // I = L^-1, column after column
#pragma unroll
                for (int i = j + 1; i < NB; i++) {
                    double v = 0.0;
#pragma unroll
                    for (int m = j; m < i; m++) v += L[i][m] * I[m][j];
                    I[i][j] = -v * I[i][i];
                }
            double* Li = B.Linv + (size_t)(c0 / NB) * NB * NB;
#pragma unroll
            for (int i = 0; i < NB; i++)
#pragma unroll
                for (int k = 0; k < NB; k++) {
                    const double v = k <= i ? I[i][k] : 0.0;
                    D[i * NB + k] = v; Li[i * NB + k] = v;
                    if (k <= i) B.Lb[(long long)(c0 + i) * M + (i - k)] = L[i][k];
                }
            if (!ok) s_fail = 1;
        }
        __syncthreads();
        if (s_fail) break;
        // panel: L[i][c0 + c] = sum_{m <= c} A[i][c0 + m] I[c][m]
        for (int idx = t; idx < r * NB; idx += COVBAND_THREADS) {
            const int ii = idx / NB, c = idx - ii * NB, i = r0 + ii;
            const double* Ar = A + (i % M) * M;
            double v = 0.0;
            for (int m = 0; m <= c; m++) v += Ar[(c0 + m) % M] * D[c * NB + m];
            Pn[ii * NB + c] = v;
            B.Lb[(long long)i * M + (i - c0 - c)] = v;
        }
        __syncthreads();
        // trailing update of the lower triangle below the block column; the NB rows entering the window take the block column's row slots
        for (int idx = t; idx < r * r; idx += COVBAND_THREADS) {
            const int ii = idx / r, jj = idx - ii * r;
            if (jj > ii) continue;
            double v = 0.0;
#pragma unroll
            for (int c = 0; c < NB; c++) v += Pn[ii * NB + c] * Pn[jj * NB + c];
            A[((r0 + ii) % M) * M + (r0 + jj) % M] -= v;
        }
        for (int idx = t; idx < NB * M; idx += COVBAND_THREADS) {
            const int q = idx / M, jj = idx - q * M, i = c0 + M + q, j = i - jj;
            if (i < n) A[(i % M) * M + j % M] = jj < bw ? B.S[(long long)i * n + j] : 0.0;
        }
        __syncthreads();
    }
    if (t == 0 && s_fail) *B.flag = 1;
}

template <int NB>
__global__ __launch_bounds__(COVBAND_THREADS) void k_cov_band_sel(CovBand B) {
    extern __shared__ double cb_lds[];
    const int n = B.n, M = B.M, bw = B.bw, t = threadIdx.x;
    if (*B.flag != 0) return;            // (uniform) the factor is not usable
    double* A = cb_lds;                  // circular image of Sigma's band, both triangles
    double* Pn = A + (size_t)M * M;      // L_Jj
    double* T = Pn + (size_t)M * NB;     // L_Jj L_jj^-1
    double* G = T + (size_t)M * NB;      // Sigma_Jj
    double* D = G + (size_t)M * NB;      // L_jj^-1
    for (int c0 = n - NB; c0 >= 0; c0 -= NB) {
        const int r0 = c0 + NB, r1 = min(n, c0 + NB + bw - 1), r = r1 - r0;
        for (int idx = t; idx < r * NB; idx += COVBAND_THREADS) {
            const int ii = idx / NB, c = idx - ii * NB, i = r0 + ii;
            Pn[idx] = B.Lb[(long long)i * M + (i - c0 - c)];
        }
        if (t < NB * NB) D[t] = B.Linv[(size_t)(c0 / NB) * NB * NB + t];
        __syncthreads();
        for (int idx = t; idx < r * NB; idx += COVBAND_THREADS) {
            const int ii = idx / NB, c = idx - ii * NB;
            double v = 0.0;
            for (int m = c; m < NB; m++) v += Pn[ii * NB + m] * D[m * NB + c];
            T[idx] = v;
        }
        __syncthreads();
        for (int idx = t; idx < r * NB; idx += COVBAND_THREADS) {
            const int ii = idx / NB, c = idx - ii * NB;
            const double* Ar = A + ((r0 + ii) % M) * M;
            double v = 0.0;
            for (int k = 0; k < r; k++) v += Ar[(r0 + k) % M] * T[k * NB + c];
            G[idx] = -v;
        }
        __syncthreads();
        // Sigma_Jj and its transpose into the image and into Sigma; Sigma_jj, lower triangle and mirror
        for (int idx = t; idx < r * NB; idx += COVBAND_THREADS) {
            const int ii = idx / NB, c = idx - ii * NB, i = r0 + ii, j = c0 + c;
            const double v = G[idx];
            A[(i % M) * M + j % M] = v; A[(j % M) * M + i % M] = v;
            B.Sig[(long long)i * n + j] = v; B.Sig[(long long)j * n + i] = v;
        }
        if (t < NB * NB) {
            const int a = t / NB, c = t - a * NB;
            if (a >= c) {
                double v = 0.0;
                for (int m = a; m < NB; m++) v += D[m * NB + a] * D[m * NB + c];
                double s = 0.0;
                for (int k = 0; k < r; k++) s += G[k * NB + a] * T[k * NB + c];
                v -= s;
                const int i = c0 + a, j = c0 + c;
                A[(i % M) * M + j % M] = v; A[(j % M) * M + i % M] = v;
                B.Sig[(long long)i * n + j] = v; B.Sig[(long long)j * n + i] = v;
            }
        }
        __syncthreads();
    }
}

// X[(x * dpf + g) * n + i] = Sigma[i][col[x] + g] for the rows i >= col[x] + dpf: L Y = E, L^T X = Y with L's band. One group of 16
// lanes per right-hand side g; lane q of the group takes the terms q, q + 16, ... of a row's sum in that order, the 16 partial sums
// are combined by a butterfly: a fixed order. The last M values of the solved vector sit in LDS; a row's entries of L are loaded one
// row ahead of their use.
__global__ __launch_bounds__(COVBAND_THREADS) void k_cov_band_cols(CovBand B, const int* __restrict__ col, double* __restrict__ X) {
    const int n = B.n, M = B.M, bw = B.bw, dpf = B.dpf, t = threadIdx.x;
    if (*B.flag != 0) return;
    __shared__ double win[COVBAND_THREADS / COVBAND_GROUP][COVBAND_MAXW];
    const int g = t / COVBAND_GROUP, q = t % COVBAND_GROUP;
    const bool act = g < dpf;
    const int cb = col[blockIdx.x];
    double* Xg = X + ((size_t)blockIdx.x * dpf + (act ? g : 0)) * n;
    double* wg = win[g];
    double lv[COVBAND_LV], ld = 0.0;
    // forward: y[i] = (e[i] - sum_{k = max(cb, i - bw + 1)}^{i - 1} L[i][k] y[k]) / L[i][i]
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
    // backward: x[i] = (y[i] - sum_{k = i + 1}^{min(n, i + bw) - 1} L[k][i] x[k]) / L[i][i], down to the first row below the block of b
    auto fetch_b = [&](int i) {
#pragma unroll
        for (int u = 0; u < COVBAND_LV; u++) {
            const int k = i + 1 + q + COVBAND_GROUP * u;
            lv[u] = (i >= 0 && k < n && k - i < bw) ? B.Lb[(long long)k * M + (k - i)] : 0.0;
        }
        ld = i >= 0 ? B.Lb[(long long)i * M] : 1.0;
    };
    fetch_b(n - 1);
    for (int i = n - 1; i >= cb + dpf; i--) {
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
            const double x = (Xg[i] - s) / d;
            wg[i % M] = x; Xg[i] = x;
        }
        __syncthreads();
    }
}

// Block e of the call's answer, dpf x dpf, at out + e * dpf^2. tab[4 e ..]: kind | r0 | c0 | x
//   0 zeros (a constant key-frame)   1 Sigma[r0 + i][c0 + j]   2 X[x][j][r0 + i]   3 X[x][i][r0 + j] (the transpose of kind 2's block)
constexpr int COVBAND_G_ZERO = 0, COVBAND_G_SIG = 1, COVBAND_G_COL = 2, COVBAND_G_COLT = 3;
__global__ __launch_bounds__(COVBAND_THREADS) void k_cov_band_gather(CovBand B, const int* __restrict__ tab, const double* __restrict__ X, double* __restrict__ out) {
    const int dpf = B.dpf, n = B.n, t = threadIdx.x;
    if (t >= dpf * dpf) return;
    const int kind = tab[4 * blockIdx.x], r0 = tab[4 * blockIdx.x + 1], c0 = tab[4 * blockIdx.x + 2], x = tab[4 * blockIdx.x + 3];
    const int i = t / dpf, j = t - i * dpf;
    double v = 0.0;
    if (kind == COVBAND_G_SIG) v = B.Sig[(long long)(r0 + i) * n + c0 + j];
    else if (kind == COVBAND_G_COL) v = X[((size_t)x * dpf + j) * n + r0 + i];
    else if (kind == COVBAND_G_COLT) v = X[((size_t)x * dpf + i) * n + r0 + j];
    out[(size_t)blockIdx.x * dpf * dpf + t] = v;
}

}  // namespace sadvio
