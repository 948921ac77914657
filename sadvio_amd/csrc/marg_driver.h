// marg_driver.h — the host side of marginalisation: the dense factorisations it is built from (pivoted / unpivoted Cholesky, the
// Jacobi eigen-solvers, the triangular inverse), sadvio_ba_marginalize as named steps
//   marg_layout -> marg_routes -> marg_assemble -> marg_invert_mm -> marg_schur -> marg_factor_cholesky | marg_factor_eigen -> marg_install
// and the bodies of sadvio_ba_marginalize_relative, sadvio_ba_sparsify, sadvio_ba_get_prior and sadvio_ba_set_prior. The kernels are marg_kernels.h's and dense_chol.h's.
// Part of the library's single translation unit (ba_capi.hip); not a public header.
#pragma once
#include "ba_handle.h"
#include "imu_host.h"
#include "solve_driver.h"

namespace {

// Diagonally pivoted Cholesky S = G^T G without data movement (marg_kernels.h: k_pchol_panel_rx / k_pchol_syrk_mma; with
// SADVIO_PCHOL_STRICT k_pchol_panel_np / k_pchol_syrk_full), in place on
// the n x n scratch S (destroyed); G (n x n) receives the factor's rows by ORIGINAL column index, h->d_jac_ints[0..n) the pivot
// step of every index (-1 = never chosen). tau >= 0: stop at pivots <= tau * max diagonal; tau < 0: at pivots <= -tau
// (absolute). Returns the rank (number of pivots taken), negative on a HIP error. One host synchronisation (the rank).
int run_pchol(sadvio_ba_handle* h, double* S, int n, double* G, double tau) {
    if (h->d_jac_ints.alloc((size_t)n + 8) != hipSuccess) return -1;
    int* piv = h->d_jac_ints.p; int* rank_d = piv + n;
    if (h->d_jac_dbl.alloc(2 * (size_t)n + 8) != hipSuccess) return -1;
    double* dg = h->d_jac_dbl.p; double* dctl = dg + 2 * (size_t)n;      // remaining diagonal | original diagonal | tau
    if (hipMemsetAsync(rank_d, 0, sizeof(int) * 8, h->stream) != hipSuccess) return -1;
    if (hipMemsetAsync(rank_d, 0xff, sizeof(int), h->stream) != hipSuccess) return -1;   // -1: still factorising
    if (hipMemsetAsync(piv, 0xff, sizeof(int) * (size_t)n, h->stream) != hipSuccess) return -1;   // done[i] = -1
    const unsigned gt = (unsigned)((n + 63) / 64);
    const bool two = n > PCH_THREADS;   // a thread owns indices i and i + 1 024: panels of 16 columns instead of 32
    const int nb = two ? 16 : 32;
    int r = -1;
    if (h->env.pchol_strict) {
        const auto panel = two ? k_pchol_panel_np<2, 16> : k_pchol_panel_np<1, 32>;
        const auto syrk = two ? k_pchol_syrk_full<16> : k_pchol_syrk_full<32>;
        for (int k0 = 0; k0 < n; k0 += nb) {
            hipLaunchKernelGGL(panel, dim3(1), dim3(PCH_THREADS), 0, h->stream, S, n, G, piv, dg, rank_d, dctl, k0, tau);
            if (k0 + nb < n) hipLaunchKernelGGL(syrk, dim3(gt, gt), dim3(256), 0, h->stream, S, n, G, rank_d, k0);
        }
        if (hipMemcpyAsync(&r, rank_d, sizeof(int), hipMemcpyDeviceToHost, h->stream) != hipSuccess || hipStreamSynchronize(h->stream) != hipSuccess) return -1;
        return r < 0 ? n : r;
    }
    // relaxed pivoting (marg_kernels.h: k_pchol_panel_rx): a panel picks its pivots up front; the first row of a panel is device state
    const auto panel = two ? k_pchol_panel_rx<2, 16> : k_pchol_panel_rx<1, 32>;
    const auto syrk = two ? k_pchol_syrk_mma<16> : k_pchol_syrk_mma<32>;
    const double safe = 1024.0 * n * 2.220446049250313e-16;
    int launched = 0;
    for (int round = 0; round < 64 && r < 0; round++) {
        const int np = round == 0 ? (n + nb - 1) / nb + 8 : 4;   // threshold pivoting leaves some panels partly filled; a launch after the end returns at once
        for (int pnl = 0; pnl < np; pnl++, launched++) {
            hipLaunchKernelGGL(panel, dim3(1), dim3(PCH_THREADS), 0, h->stream, S, n, G, piv, dg, rank_d, dctl, launched == 0 ? 1 : 0, tau, safe);
            hipLaunchKernelGGL(syrk, dim3(gt, gt), dim3(256), 0, h->stream, S, n, G, rank_d);
        }
        if (hipMemcpyAsync(&r, rank_d, sizeof(int), hipMemcpyDeviceToHost, h->stream) != hipSuccess || hipStreamSynchronize(h->stream) != hipSuccess) return -1;
    }
    if ((h->env.debug & 16384)) {
        int c8[8];
        if (hipMemcpy(c8, rank_d, sizeof(c8), hipMemcpyDeviceToHost) == hipSuccess)
            fprintf(stderr, "[sadvio dbg] relaxed pivoted cholesky n %d rank %d: %d panels launched, %d ran (%d strict), %d candidates skipped\n", n, r, launched, c8[3] + 1, c8[4], c8[5]);
    }
    return r < 0 ? -1 : r;
}

// Block one-sided Jacobi on the r rows (length n, packed) of G until they are mutually orthogonal: the rows converge to
// sqrt(lambda_i) u_i^T of G^T G. Returns the number of sweeps (negative = HIP error). One host synchronisation per sweep.
int run_jacobi_rows(sadvio_ba_handle* h, double* G, int r, int n, int* flag) {
    const bool mma = n <= JM_MAXN;   // blocks of JM rows on the matrix cores; longer rows: the VALU version on blocks of JB rows
    const int ldx = jm_ldx(n);
    const size_t jm_lds = (size_t)JM2 * ldx * sizeof(double);
    if (mma && hipFuncSetAttribute((const void*)k_jacobi_mma, hipFuncAttributeMaxDynamicSharedMemorySize, (int)jm_lds) != hipSuccess) return -1;
    const int jb = mma ? JM : JB;
    const int nb = (r + jb - 1) / jb, nbpad = nb + (nb & 1);
    const double jtol = h->env.jacobi_tol;   // |g_p . g_q| <= jtol |g_p| |g_q| ends a pair
    int sweeps = 0;
    long long* jts = nullptr;   // phase timestamps of one launch (SADVIO_KERNEL_TS builds, SADVIO_DEBUG & 4096)
    if ((h->env.debug & 4096) && n > 500 && h->d_dbg.alloc(DBG_SLOTS) == hipSuccess) jts = h->d_dbg.p + 44;
    for (; sweeps < 40 && nbpad >= 2; sweeps++) {
        if (hipMemsetAsync(flag, 0, sizeof(int), h->stream) != hipSuccess) return -1;
        for (int st = 0; st < nbpad - 1; st++) {
            long long* ts = sweeps == 0 && st == 3 ? jts : nullptr;
            if (mma) hipLaunchKernelGGL(k_jacobi_mma, dim3(nbpad / 2), dim3(JAC_THREADS), jm_lds, h->stream, G, r, n, ldx, nbpad, st, jtol, flag, ts);
            else hipLaunchKernelGGL(k_jacobi_block<8>, dim3(nbpad / 2), dim3(JAC_THREADS), 0, h->stream, G, r, n, nbpad, st, jtol, flag);   // n <= PCH_MAXN = 8 * JAC_THREADS
        }
        int f = 0;
        if (hipMemcpyAsync(&f, flag, sizeof(int), hipMemcpyDeviceToHost, h->stream) != hipSuccess || hipStreamSynchronize(h->stream) != hipSuccess) return -1;
        if ((h->env.debug & 16384)) fprintf(stderr, "[sadvio dbg] block jacobi n %d rank %d sweep %d block pairs rotated %d\n", n, r, sweeps, f);
        if (!f) { sweeps++; break; }
    }
    if (jts) {
        long long t8[8];
        if (hipMemcpy(t8, jts, sizeof(t8), hipMemcpyDeviceToHost) == hipSuccess) {
            fprintf(stderr, "[sadvio dbg] k_jacobi_mma phases (us, cumulative): gram | update loads issued | barrier | M | check | inner sweep | end:");
            for (int i = 1; i < 8; i++) fprintf(stderr, " %.2f", (t8[i] - t8[0]) * 0.01);
            fprintf(stderr, "\n");
        }
    }
    return sweeps;
}

// pivot tolerance of the rank-revealing Cholesky for an eigenvalue-cut mode: the noise floor's pivots end at 4 n eps of the
// largest one (the null space of a marginalisation prior sits exactly there); the reference's absolute 1e-12 (Marginalization::
// _eps) becomes a pivot floor of 1e-12 / n — a remaining eigenvalue above 1e-12 keeps the remaining trace, hence the largest
// remaining diagonal entry, above it.
double pchol_tau(int n, int eig_cut_mode) {
    return eig_cut_mode == SADVIO_EIG_CUT_NOISE_FLOOR ? 4.0 * n * 2.220446049250313e-16 : -1e-12 / std::max(n, 1);
}

// Unpivoted Cholesky of the symmetric positive definite n x n matrix whose lower triangle sits in V (leading dimension n; destroyed)
// by the wide-panel solver of the dense reduced systems (launch_wfac), the vector y riding along as its right-hand side (-> L^-1 y).
// Lx (n x n): the panels; Ltw: ceil(n / 96) * (WD_LT + 6 * 256) doubles for
// the diagonal blocks' tiles and their re-inverted diagonal tiles; A0 (leading dimension ld0): the original matrix, for the pivot test
// (k_wfac_diag). Returns 1 = every pivot is safely positive (the factor is in Lx / Ltw, packed by k_wfac_pack), 0 = not (the caller
// takes the rank-revealing route), -1 = HIP error. One host synchronisation.
int run_wfac(sadvio_ba_handle* h, double* V, int n, double* y, double* Lx, double* Ltw, const double* A0, long long ld0, double tau_rel, double* dmax, int* info) {
    const int nsteps = (n + WD - 1) / WD;
    double* Ld = Ltw + (size_t)nsteps * WD_LT;
    if (hipMemsetAsync(info, 0, sizeof(int) * 2, h->stream) != hipSuccess) return -1;
    launch_wfac(h, V, (long long)n, n, y, Lx, Ltw, nullptr, info, nullptr, nullptr);
    hipLaunchKernelGGL(k_diag_max, dim3(1), dim3(256), 0, h->stream, A0, ld0, n, dmax);
    hipLaunchKernelGGL(k_wfac_diag, dim3(nsteps * WD_T), dim3(64), 0, h->stream, Ltw, n, A0, ld0, tau_rel, dmax, 1024.0 * n * 2.220446049250313e-16, Ld, info + 1);
    int st2[2] = {0, 0};
    if (hipMemcpyAsync(st2, info, sizeof(st2), hipMemcpyDeviceToHost, h->stream) != hipSuccess || hipStreamSynchronize(h->stream) != hipSuccess) return -1;
    return st2[0] == 0 && st2[1] == 0 ? 1 : 0;
}
size_t wfac_scratch_doubles(int n) { return (size_t)((n + WD - 1) / WD) * (WD_LT + WD_T * 256) + 8; }

// one-sided Jacobi eigen-decomposition of the symmetric n x n block at A (leading dimension lda): G, V (n x n each)
// and ev (n) are device buffers; returns the number of sweeps (negative = HIP error)
int run_jacobi(sadvio_ba_handle* h, const double* A, long long lda, int n, int lower_only, double* G, double* V, double* ev, int* flag, int eig_cut_mode) {
    const long long nn = (long long)n * n;
    // Cholesky-preconditioned block Jacobi (marg_kernels.h): sym(A) -> V (scratch), pivoted Cholesky V -> G = L^T, block
    // one-sided Jacobi sweeps on the rows of G, then eigen-pairs from the rows -> V, ev
    if (n >= 32 && n <= PCH_MAXN) {
        hipLaunchKernelGGL(k_jacobi_init, dim3((unsigned)((nn + 255) / 256)), dim3(256), 0, h->stream, A, lda, n, V, G, lower_only);
        const int r = run_pchol(h, V, n, G, pchol_tau(n, eig_cut_mode));
        if (r < 0) return -1;
        const int sweeps = run_jacobi_rows(h, G, r, n, flag);
        if (sweeps < 0) return -1;
        hipLaunchKernelGGL(k_eig_from_rows, dim3(n), dim3(JAC_THREADS), 0, h->stream, G, h->d_jac_ints.p + n, n, V, ev);
        return sweeps;
    }
    hipLaunchKernelGGL(k_jacobi_init, dim3((unsigned)((nn + 255) / 256)), dim3(256), 0, h->stream, A, lda, n, G, V, lower_only);
    const int npad = n + (n & 1);
    // noise floor of the column norms (see k_jacobi_floor); flag[2..3] = max norm bits, flag[4..5] = the floor
    unsigned long long* amax = (unsigned long long*)(flag + 2);
    double* floor2 = (double*)(flag + 4);
    if (hipMemsetAsync(flag, 0, 8 * sizeof(int), h->stream) != hipSuccess) return -1;
    if (n > 0 && eig_cut_mode == SADVIO_EIG_CUT_NOISE_FLOOR) {   // the reference's cut sits below that floor: every pair keeps rotating
        hipLaunchKernelGGL(k_jacobi_floor, dim3(n), dim3(JAC_THREADS), 0, h->stream, G, n, amax, floor2, 0);
        hipLaunchKernelGGL(k_jacobi_floor, dim3(1), dim3(JAC_THREADS), 0, h->stream, G, n, amax, floor2, 1);
    }
    int sweeps = 0;
    for (; sweeps < 40 && npad >= 2; sweeps++) {
        if (hipMemsetAsync(flag, 0, sizeof(int), h->stream) != hipSuccess) return -1;
        for (int s = 0; s < npad - 1; s++)
            hipLaunchKernelGGL(k_jacobi_step, dim3(npad / 2), dim3(JAC_THREADS), 0, h->stream, G, V, n, npad, s, 1e-14, flag, floor2);
        int f = 0;
        if (hipMemcpyAsync(&f, flag, sizeof(int), hipMemcpyDeviceToHost, h->stream) != hipSuccess) return -1;
        if (hipStreamSynchronize(h->stream) != hipSuccess) return -1;
        if ((h->env.debug & 16384)) fprintf(stderr, "[sadvio dbg] jacobi n %d sweep %d rotations %d\n", n, sweeps, f);
        if (!f) { sweeps++; break; }
    }
    hipLaunchKernelGGL(k_jacobi_eigenvalues, dim3(n), dim3(JAC_THREADS), 0, h->stream, G, V, n, ev);
    return sweeps;
}

// The reference cuts by EIGENVALUE (lambda > 1e-12, marginalization.cpp:318-342, marginalization.hpp:58); the rank-revealing Cholesky
// cuts by pivot, at the floor 1e-12 / n that never drops an eigenvalue above the cut — and therefore keeps directions whose
// eigenvalue lies below it (lambda_min <= the last pivot d <= ~n lambda_min). For the trailing pivots inside that band the small
// eigenvalues are evaluated the way the eigenvalue test means them: with G in pivot order (upper triangular) and x_s = G^-1 e_s for the
// k trailing steps, the k smallest eigenvalues of A = G^T G are, to O(d / gap) relative, the reciprocals of the eigenvalues of X^T X
// (A^-1 = G^-1 G^-T is dominated by those columns; k = 1: lambda = d / (1 + |w|^2), the Rayleigh quotient of the near-null vector) —
// relatively accurate where an eigen-decomposition of A in double precision only returns noise of size eps |A|. Rows whose eigenvalue
// is <= 1e-12 are dropped from the end. The solves run on the device (k_rank_backsub), the k x k eigenproblem on the host, on guarded calls only (a trailing pivot below
// RANK_GUARD x 1e-12: one call in 25 in the sliding sequences). Returns the refined rank, -1 on a HIP error.
constexpr double RANK_GUARD = 1e4;
int refine_rank_by_eigenvalue(sadvio_ba_handle* h, const double* G, int n1, int nf) {
    constexpr int KMAX = 8;              // trailing pivots looked at
    const int nl = std::min(nf, KMAX);
    std::vector<int> step_of(n1);
    if (hipMemcpyAsync(step_of.data(), h->d_jac_ints.p, sizeof(int) * (size_t)n1, hipMemcpyDeviceToHost, h->stream) != hipSuccess) return -1;
    std::vector<double> last((size_t)nl * n1);      // the last rank rows: their diagonal entries are the trailing pivots
    if (hipMemcpyAsync(last.data(), G + (size_t)(nf - nl) * n1, sizeof(double) * (size_t)nl * n1, hipMemcpyDeviceToHost, h->stream) != hipSuccess) return -1;
    if (hipStreamSynchronize(h->stream) != hipSuccess) return -1;
    std::vector<int> col_of(nf, -1);                  // pivot column of every step
    for (int c = 0; c < n1; c++) if (step_of[c] >= 0 && step_of[c] < nf) col_of[step_of[c]] = c;
    for (int s = 0; s < nf; s++) if (col_of[s] < 0) return nf;    // (cannot happen: every step has its column)
    auto gd = [&](int s) { return last[(size_t)(s - (nf - nl)) * n1 + col_of[s]]; };   // diagonal of the factor in pivot order, s >= nf - nl
    const double d_last = gd(nf - 1) * gd(nf - 1);
    if (h->env.debug) fprintf(stderr, "[sadvio dbg] rank refinement: last pivot %.3e (rank %d of %d)\n", d_last, nf, n1 - 1);
    if (!(d_last <= RANK_GUARD * 1e-12)) return nf;
    int k = 0;
    while (k < nl) { const double dv = gd(nf - 1 - k); if (dv * dv <= RANK_GUARD * 1e-12) k++; else break; }
    // guarded: x_q = G^-1 e_s, s = nf - 1 - q, by k_rank_backsub on the device (one workgroup per vector; 0.29 ms with the read-back at n = 915, k = 4)
    const auto tq0 = std::chrono::steady_clock::now();
    if (h->d_rank_col.alloc((size_t)nf) != hipSuccess || h->d_rank_x.alloc((size_t)k * nf) != hipSuccess) return -1;
    if (hipMemcpyAsync(h->d_rank_col.p, col_of.data(), sizeof(int) * (size_t)nf, hipMemcpyHostToDevice, h->stream) != hipSuccess) return -1;
    hipLaunchKernelGGL(k_rank_backsub, dim3(k), dim3(RB_THREADS), 0, h->stream, G, n1, h->d_rank_col.p, nf - 1, nf, h->d_rank_x.p);   // one workgroup per vector
    std::vector<double> Xall((size_t)k * nf);
    if (hipMemcpyAsync(Xall.data(), h->d_rank_x.p, sizeof(double) * (size_t)k * nf, hipMemcpyDeviceToHost, h->stream) != hipSuccess) return -1;
    if (hipStreamSynchronize(h->stream) != hipSuccess) return -1;
    std::vector<std::vector<double>> X(k, std::vector<double>(nf, 0.0));
    for (int q = 0; q < k; q++) std::copy(Xall.begin() + (size_t)q * nf, Xall.begin() + (size_t)q * nf + (nf - q), X[q].begin());   // rows above s = nf - 1 - q are not written: x is zero there
    const auto tq1 = std::chrono::steady_clock::now();
    // eigenvalues of the k x k Gram matrix X^T X (cyclic Jacobi); lambda_small(A) = 1 / them
    std::vector<double> B((size_t)k * k);
    for (int a = 0; a < k; a++) for (int b = 0; b < k; b++) { double acc = 0.0; for (int i = 0; i < nf; i++) acc += X[a][i] * X[b][i]; B[(size_t)a * k + b] = acc; }
    for (int sweep = 0; sweep < 30 && k > 1; sweep++) {
        double off = 0.0;
        for (int a = 0; a < k; a++) for (int b = a + 1; b < k; b++) {
            const double apq = B[(size_t)a * k + b];
            off += apq * apq;
            if (apq == 0.0) continue;
            const double th = (B[(size_t)b * k + b] - B[(size_t)a * k + a]) / (2.0 * apq);
            const double t = (th >= 0 ? 1.0 : -1.0) / (std::fabs(th) + std::sqrt(th * th + 1.0)), c = 1.0 / std::sqrt(t * t + 1.0), sn = t * c;
            for (int i = 0; i < k; i++) { const double u = B[(size_t)i * k + a], v = B[(size_t)i * k + b]; B[(size_t)i * k + a] = c * u - sn * v; B[(size_t)i * k + b] = sn * u + c * v; }
            for (int i = 0; i < k; i++) { const double u = B[(size_t)a * k + i], v = B[(size_t)b * k + i]; B[(size_t)a * k + i] = c * u - sn * v; B[(size_t)b * k + i] = sn * u + c * v; }
        }
        if (off <= 1e-30 * B[0] * B[0]) break;
    }
    int drop = 0;
    for (int a = 0; a < k; a++) if (!(1.0 / B[(size_t)a * k + a] > 1e-12)) drop++;
    if (h->env.debug) fprintf(stderr, "[sadvio dbg] rank refinement: %d vector(s), device back-substitution + read-back %.3f ms, host %.3f ms\n", k, std::chrono::duration<double, std::milli>(tq1 - tq0).count(), std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - tq1).count());
    if ((h->env.debug & 16384) || drop) {
        h->marg_stats[3] += drop ? 1 : 0;
        if (h->env.debug) {
            fprintf(stderr, "[sadvio dbg] rank refinement: %d trailing pivot(s) below %.0e, eigenvalue estimates", k, RANK_GUARD * 1e-12);
            for (int a = 0; a < k; a++) fprintf(stderr, " %.3e", 1.0 / B[(size_t)a * k + a]);
            fprintf(stderr, " -> %d dropped (rank %d of %d)\n", drop, nf - drop, n1 - 1);
        }
    }
    if (drop) {   // the packing kernels read the rank from the device (k_marg_pack_chol)
        const int r2 = nf - drop;
        if (hipMemcpy(h->d_jac_ints.p + n1, &r2, sizeof(int), hipMemcpyHostToDevice) != hipSuccess) return -1;
    }
    return nf - drop;
}

// eigenvalue cut of the pseudo-inverse / rank-revealing decomposition (sadvio_ba.h: SADVIO_EIG_CUT_*): the reference's absolute
// 1e-12 (marginalization.hpp:58, applied at marginalization.cpp:237,322), or that constant with the rounding-noise floor
// n eps lambda_max (see oracle/marg.c)
double marg_cut(const std::vector<double>& ev, int eig_cut_mode) {
    if (eig_cut_mode != SADVIO_EIG_CUT_NOISE_FLOOR) return 1e-12;
    double mx = 0.0;
    for (double v : ev) mx = std::max(mx, std::fabs(v));
    return std::max(1e-12, (double)ev.size() * 2.220446049250313e-16 * mx);
}

inline void launch_mgemm(sadvio_ba_handle* h, double* C, long long ldc, const double* A, long long sai, long long sak, const double* B, long long sbk,
                         long long sbj, int M, int N, int K, double alpha, double beta) {
    hipLaunchKernelGGL(k_mgemm, dim3((N + 63) / 64, (M + 63) / 64), dim3(256), 0, h->stream, C, ldc, A, sai, sak, B, sbk, sbj, M, N, K, alpha, beta);
}

// Z (n_full x n) with Z^T Z = Sigma_k = pseudo-inverse of the prior's information, for the NFR covariances of sparsify:
// eigen form: rows J_c / lambda_c; Cholesky form of full rank: the triangular inverse of G (k_tri_*: recursive halving on the
// matrix cores); a rank-deficient Cholesky-form prior is first orthogonalised by the block Jacobi (its rows then ARE the eigen form).
int prior_build_Z(sadvio_ba_handle* h, const double* J, int nf, int n, int form, const int* step_of, double* Z, int cut_mode, double* trace_out = nullptr, bool guard = false) {
    MargScratch& M = h->mg;
    bool hidden = false;    // guard: the inverse shows an eigenvalue that may lie below the reference's cut -> pseudo-inverse by orthogonalised rows
    if (form == SADVIO_PRIOR_FORM_CHOLESKY && nf == n) {
        const int npad = (n + 31) / 32 * 32;
        HIP_TRY(M.L.alloc((size_t)npad * npad)); HIP_TRY(M.Tb.alloc((size_t)npad * npad)); HIP_TRY(M.piv_of.alloc(n));
        MargScratch::TriPlan& TP = M.tri_plans[npad];
        if (TP.leaves == 0) {
            // node table of the recursion over [0, npad): leaves of <= 32 rows, inner nodes grouped by height
            std::vector<std::vector<TriNode>> lev;
            std::vector<TriNode> leaves;
            struct Rec { static int go(int lo, int hi, std::vector<std::vector<TriNode>>& lev, std::vector<TriNode>& leaves) {
                if (hi - lo <= 32) { leaves.push_back({lo, lo, hi, 0}); return 0; }
                const int blocks = (hi - lo + 31) / 32, mid = lo + 32 * ((blocks + 1) / 2);
                const int hl = go(lo, mid, lev, leaves), hr = go(mid, hi, lev, leaves);
                const int ht = std::max(hl, hr) + 1;
                if ((int)lev.size() < ht) lev.resize(ht);
                lev[ht - 1].push_back({lo, mid, hi, 0});
                return ht;
            } };
            Rec::go(0, npad, lev, leaves);
            std::vector<TriNode> all(leaves);
            TP.levels.clear();
            for (auto& l : lev) {
                int mm = 0, mn = 0;
                for (auto& nd : l) { mm = std::max(mm, nd.hi - nd.mid); mn = std::max(mn, nd.mid - nd.lo); }
                TP.levels.push_back({(int)all.size(), (int)l.size(), mm, mn});
                all.insert(all.end(), l.begin(), l.end());
            }
            TP.leaves = (int)leaves.size();
            HIP_TRY(TP.nodes.alloc(all.size()));
            h->up.add(TP.nodes.p, all.data(), all.size() * sizeof(TriNode));
            HIP_TRY(h->up.flush(h->stream));
        }
        hipLaunchKernelGGL(k_tri_gather, dim3((n + 255) / 256), dim3(256), 0, h->stream, J, n, step_of, M.piv_of.p, npad, M.L.p, 0);
        const long long np2 = (long long)npad * npad;
        hipLaunchKernelGGL(k_tri_gather, dim3((unsigned)((np2 + 255) / 256)), dim3(256), 0, h->stream, J, n, step_of, M.piv_of.p, npad, M.L.p, 1);
        hipLaunchKernelGGL(k_tri_leaf, dim3(TP.leaves), dim3(64), 0, h->stream, M.L.p, npad, TP.nodes.p);
        for (const auto& lv : TP.levels) {
            const dim3 grid((lv.max_n + 63) / 64, (lv.max_m + 63) / 64, lv.count);
            hipLaunchKernelGGL(k_tri_level, grid, dim3(256), 0, h->stream, M.L.p, M.Tb.p, npad, TP.nodes.p + lv.first, 0);
            hipLaunchKernelGGL(k_tri_level, grid, dim3(256), 0, h->stream, M.L.p, M.Tb.p, npad, TP.nodes.p + lv.first, 1);
        }
        const long long nn = (long long)n * n;
        hipLaunchKernelGGL(k_tri_scatter, dim3((unsigned)((nn + 255) / 256)), dim3(256), 0, h->stream, M.L.p, npad, n, step_of, Z);
        if (trace_out || (guard && cut_mode == SADVIO_EIG_CUT_REFERENCE)) {
            // trace(A^-1) = |Z|_F^2 bounds the smallest eigenvalue of A = G^T G from below (lambda_min >= 1 / trace): pivots that all pass do
            // not (they bound eigenvalues from above). Callers: Amm's pseudo-inverse in marginalize (trace_out), Sigma_k of sparsify (guard)
            HIP_TRY(M.lam.alloc((size_t)n + 2));
            hipLaunchKernelGGL(k_row_norm2, dim3(n), dim3(JAC_THREADS), 0, h->stream, Z, n, n, M.lam.p);
            std::vector<double> rn(n);
            HIP_TRY(hipMemcpyAsync(rn.data(), M.lam.p, sizeof(double) * (size_t)n, hipMemcpyDeviceToHost, h->stream));
            HIP_TRY(hipStreamSynchronize(h->stream));
            double tr = 0.0;
            for (int i = 0; i < n; i++) tr += rn[i];
            if (h->env.debug & 16384) fprintf(stderr, "[sadvio dbg] triangular inverse: trace(A^-1) %.3e (n %d): lambda_min >= %.3e\n", tr, n, 1.0 / tr);
            if (trace_out) *trace_out = tr;
            hidden = guard && cut_mode == SADVIO_EIG_CUT_REFERENCE && !(tr < 1e12);
            if (hidden) h->hidden_eig_count++;
        }
        if (!hidden) return SADVIO_OK;
    }
    const double* rows = J;
    if (form == SADVIO_PRIOR_FORM_CHOLESKY) {   // rank-deficient (or an eigenvalue that may lie below the cut): orthogonalise a copy of the rows
        HIP_TRY(M.G.alloc((size_t)nf * n)); HIP_TRY(M.flag.alloc(8));
        HIP_TRY(hipMemcpyAsync(M.G.p, J, sizeof(double) * (size_t)nf * n, hipMemcpyDeviceToDevice, h->stream));
        if (run_jacobi_rows(h, M.G.p, nf, n, M.flag.p) < 0) { h->err = "sparsify: HIP error in the eigen-solver"; return SADVIO_E_HIP; }
        rows = M.G.p;
    }
    HIP_TRY(M.lam.alloc((size_t)nf + 2));
    hipLaunchKernelGGL(k_row_norm2, dim3(nf), dim3(JAC_THREADS), 0, h->stream, rows, nf, n, M.lam.p);
    hipLaunchKernelGGL(k_z_cut, dim3(1), dim3(256), 0, h->stream, M.lam.p, nf, cut_mode == SADVIO_EIG_CUT_NOISE_FLOOR ? 1 : 0, M.lam.p + nf);
    hipLaunchKernelGGL(k_z_from_eig, dim3(nf), dim3(JAC_THREADS), 0, h->stream, rows, n, M.lam.p, M.lam.p + nf, Z);
    return SADVIO_OK;
}

// ---- sadvio_ba_marginalize ---------------------------------------------------------------------------------------------------

// Index layout of one call (marginalization.cpp:38-113) and the host-side lists of its blocks; the per-landmark columns, the item
// lists and the previous prior's column map live in the handle's MargScratch (lcol, items, col).
struct MargLayout {
    int m = 0, n = 0, N = 0;     // marginalised | kept columns, N = m + n
    int kf_keep_col = -1;        // first column of the kept key-frame (-1: none)
    int n_items = 0;             // reprojection factors seen from frame0
    int nl = 0, nfl = 0;         // previous prior: columns, rows (0: none)
    bool last_resident = false;  // ... and it is the handle's (no upload)
    MargSmall S{};               // IMU factor + bias factor, pose priors
};

enum class LastScatter { none, resident_hg, gemm, small };   // how the previous prior's J^T J, J^T r0 reach A, b

// Which routes a call may take. Everything here follows from the request, the sizes, PriorState and EnvCfg: it is decided once,
// behind marg_layout, and the steps read it.
struct MargRoutes {
    bool chol_form;          // the new prior in Cholesky form (else: the reference's eigen form)
    // the resident prior still carries the Ak / bk it was factorised from: J^T J and J^T r0 without touching J (resident_hg);
    // else H = J^T J on the matrix cores (gemm, nl >= 64) or one thread per entry (small)
    LastScatter last;
    // ---- Schur complement with the pseudo-inverse of Amm (marginalization.cpp:234-248) ----------------------------------
    // A well-conditioned Amm (every pivot of the rank-revealing Cholesky above the noise floor: the usual case — frame0's states and
    // its lonely stereo landmarks are fully observed) has Amm^+ = Amm^-1 under either cut, and the inverse comes from the triangular
    // inverse of that factor (Z^T Z, k_tri_*): 0.3 ms instead of ~1.1 ms of Jacobi launches. Anything else takes the reference's
    // eigen-decomposition with the request's cut.
    // ... but only where the inverse itself PROVES that no eigenvalue of Amm lies below the reference's cut (round 6). Pivots bound
    // eigenvalues from above only: behind a rank-deficient previous prior frame0's block can carry an eigenvalue below 1e-12 under pivots
    // that all pass, and where the reference's pseudo-inverse zeroes that direction (marginalization.cpp:234-240) an inverse divides by it
    // — step 13 of the config-3-size dense sequence (previous prior 917 of 918): Ak lost 9 187 of information along the kept frame's
    // rotation, 1e-6 in the next solve's poses (tests/test_gpu_sliding_full_size.py; found by marginalising the device's own window
    // with the oracle, scripts/sliding_same_inputs_marg.py). The proof: lambda_min(Amm) >= 1 / trace(Amm^-1), and trace(Amm^-1) =
    // |Z|_F^2 of the triangular inverse the route forms anyway (m row norms, one read-back; 2.3e13 at that step, 1e3 .. 5e11 at the other
    // 24). A trace of 1e12 or more sends the call to the reference's eigen-decomposition with the request's cut. (Gating on the previous
    // prior's rank instead was measured too: it sends full-rank blocks through the eigen route as well, whose inverse agrees with the
    // oracle's to 4e-9 where the Cholesky inverse agrees to 1e-11 — the sequence's worst step 3e-7 instead of 1.3e-8.)
    // Amm is positive definite whenever frame0 carries a prior or enough observations: unpivoted wide-panel factor first (run_wfac)
    bool mm_unpivoted;
    bool mm_pivoted;         // the rank-revealing factor of Amm, where the unpivoted one was not tried or a pivot of it failed
    // (without an earlier prior frame1's velocity / bias directions are only held relative to frame0's: Ak is rank deficient, the
    // attempt would be wasted; SADVIO_MARG_UNPIVOTED=1 tries it regardless)
    // Only under the reference's absolute cut: an unpivoted factorisation is not rank revealing (the pivot of the last index of a
    // dependent set is lambda / v_i^2, v = the null vector - any size), so the noise-floor mode, whose point is a reliable
    // numerical rank, always takes the pivoted route; under the absolute 1e-12 cut both routes keep every direction whose pivot is
    // positive, as the reference's eigenvalue test does.
    // ... and only behind a previous prior of FULL rank (round 6): a prior that dropped a direction hands its near-null direction on to
    // the next Ak, where the unpivoted pivots do not show it (measured, step 13 of the VIO dense sliding sequence: eigenvalue 1.1e-14 —
    // below the reference's cut — under pivots that all pass; profiles/r06_rank_arbiter.txt).
    bool k_unpivoted;
};

MargRoutes marg_routes(const sadvio_ba_handle* h, const sadvio_marg_request* rq, const MargLayout& L) {
    const bool ref_cut = rq->eig_cut_mode == SADVIO_EIG_CUT_REFERENCE;
    MargRoutes R{};
    R.chol_form = rq->prior_form == SADVIO_PRIOR_FORM_CHOLESKY;
    R.last = L.nfl <= 0 ? LastScatter::none : (L.last_resident && h->prior.hg_valid) ? LastScatter::resident_hg : L.nl >= 64 ? LastScatter::gemm : LastScatter::small;
    R.mm_unpivoted = !h->env.marg_pivoted && ref_cut;
    R.mm_pivoted = L.m >= 32 && L.m <= PCH_MAXN;
    R.k_unpivoted = R.chol_form && !h->env.marg_pivoted && ref_cut && ((rq->last_n_full != 0 && L.nfl == L.nl) || h->env.marg_unpivoted);
    return R;
}

// 1. Validate the request, lay out the columns, list the blocks. Host work only (and hipSetDevice): nothing is allocated or queued
// before the request is known to be good.
int marg_layout(sadvio_ba_handle* h, int w, const sadvio_marg_request* rq, MargLayout& L, sadvio_marg_result* res, int32_t* lmk_col_out) {
    const WinDev& d = h->plan.wins[w].d;
    if (rq->kf_marg < 0 || rq->kf_marg >= d.n_kf || rq->kf_keep >= d.n_kf || rq->n_marg < 0 || rq->n_keep < 0 || rq->n_prior < 0 ||
        rq->n_prior > 4 || (rq->n_marg > 0 && !rq->lmk_marg) || (rq->n_keep > 0 && !rq->lmk_keep) || (rq->n_prior > 0 && !rq->priors) ||
        (rq->eig_cut_mode != SADVIO_EIG_CUT_REFERENCE && rq->eig_cut_mode != SADVIO_EIG_CUT_NOISE_FLOOR) ||
        (rq->prior_form != SADVIO_PRIOR_FORM_EIGEN && rq->prior_form != SADVIO_PRIOR_FORM_CHOLESKY)) {
        h->err = "marginalize: request out of range"; return SADVIO_E_INVALID_ARG;
    }
    HIP_TRY(hipSetDevice(h->device));
    MargScratch& M = h->mg;
    PriorState& PR = h->prior;
    // index layout, marginalization.cpp:38-113
    const int m = L.m = 6 + (rq->marg_has_imu ? 9 : 0) + 3 * rq->n_marg;
    const int n = L.n = (rq->kf_keep >= 0 ? 15 : 0) + 3 * rq->n_keep;
    L.N = m + n;
    std::vector<int>& lcol = M.lcol;
    lcol.assign(std::max(d.n_lmk, 1), -1);
    int idx = 6 + (rq->marg_has_imu ? 9 : 0);
    for (int k = 0; k < rq->n_marg; k++) {
        if (rq->lmk_marg[k] < 0 || rq->lmk_marg[k] >= d.n_lmk) { h->err = "marginalize: landmark index out of range"; return SADVIO_E_INVALID_ARG; }
        lcol[rq->lmk_marg[k]] = idx; idx += 3;
    }
    int kf_keep_col = -1;
    if (rq->kf_keep >= 0) { kf_keep_col = idx; idx += 15; }
    L.kf_keep_col = kf_keep_col;
    for (int k = 0; k < rq->n_keep; k++) {
        if (rq->lmk_keep[k] < 0 || rq->lmk_keep[k] >= d.n_lmk) { h->err = "marginalize: landmark index out of range"; return SADVIO_E_INVALID_ARG; }
        lcol[rq->lmk_keep[k]] = idx; idx += 3;
    }
    if (res) { res->m = m; res->n = n; res->n_full = 0; res->kf_col = kf_keep_col >= 0 ? kf_keep_col - m : -1; res->sweeps_mm = res->sweeps_k = 0; }
    if (lmk_col_out) for (int k = 0; k < rq->n_keep; k++) lmk_col_out[k] = lcol[rq->lmk_keep[k]] - m;
    if (n < 4) {   // the reference clears its prior state too (…Analytic.cpp:620-625)
        PR.valid = false; PR.z_valid = false; PR.hg_valid = false; PR.serial++;
        h->err = "marginalize: fewer than 4 kept columns, refused (marginalization.cpp:215-216)"; return SADVIO_E_REFUSED;
    }
    if (rq->prior_form == SADVIO_PRIOR_FORM_CHOLESKY && n + 1 > PCH_MAXN) { h->err = "marginalize: the Cholesky form handles n < 2048"; return SADVIO_E_INVALID_ARG; }
    // reprojection factors of kept then marginalised landmarks seen from frame0
    std::vector<int>& it2 = M.items; std::vector<int>& itl = M.items_l;
    it2.clear(); itl.clear();
    for (int pass = 0; pass < 2; pass++) {
        const int cnt = pass == 0 ? rq->n_keep : rq->n_marg;
        const int32_t* list = pass == 0 ? rq->lmk_keep : rq->lmk_marg;
        for (int k = 0; k < cnt; k++) {
            const int gl = d.lmk_base + list[k];
            for (int o = h->plan.lmk_ob[gl]; o < h->plan.lmk_oe[gl]; o++)
                if (h->plan.obs_kf[o] == d.kf_base + rq->kf_marg && h->plan.obs_perm[o] >= 0) { it2.push_back(o); it2.push_back(lcol[list[k]]); itl.push_back(gl); }  // pseudo-observations excluded
        }
    }
    L.n_items = (int)itl.size();
    it2.insert(it2.end(), itl.begin(), itl.end());
    // IMU factor + bias factor, pose priors
    MargSmall& S = L.S;
    if (rq->imu && rq->kf_keep >= 0 && rq->marg_has_imu) {
        sadvio_imu_factor f = *rq->imu;
        f.kf_i = rq->kf_marg; f.kf_j = rq->kf_keep;
        if (!make_imu_dev(f, d.kf_base, S.imu)) { h->err = "marginalize: IMU covariance is not positive definite"; return SADVIO_E_INVALID_ARG; }
        S.has_imu = 1; S.kf_i = d.kf_base + rq->kf_marg; S.kf_j = d.kf_base + rq->kf_keep; S.kf_keep_col = kf_keep_col;
    }
    for (int k = 0; k < rq->n_prior; k++) {
        const sadvio_pose_prior& pr = rq->priors[k];
        const int base = pr.kf == rq->kf_marg ? 0 : (pr.kf == rq->kf_keep ? kf_keep_col : -1);
        if (base < 0) continue;
        const int q = S.n_prior++;
        S.prior_kf[q] = d.kf_base + pr.kf; S.prior_base[q] = base;
        memcpy(S.prior_T[q], pr.T_prior, sizeof(S.prior_T[q])); memcpy(S.prior_inf[q], pr.inf_diag, sizeof(S.prior_inf[q]));
    }
    // previous prior at zero deltas: the handle's (no upload) or the caller's arrays
    int nl = 0, nfl = 0;
    if (rq->last_n_full == SADVIO_PRIOR_RESIDENT) {
        if (!PR.valid) { h->err = "marginalize: last_n_full = SADVIO_PRIOR_RESIDENT but the handle holds no prior"; return SADVIO_E_STATE; }
        nl = PR.n; nfl = PR.n_full; L.last_resident = true;
    } else if (rq->last_n_full > 0) {
        nl = rq->last_n; nfl = rq->last_n_full;
        if (!rq->last_J || !rq->last_r0 || nl <= 0) { h->err = "marginalize: previous prior arrays missing"; return SADVIO_E_INVALID_ARG; }
    } else if (rq->last_n_full < 0) { h->err = "marginalize: last_n_full < 0"; return SADVIO_E_INVALID_ARG; }
    L.nl = nl; L.nfl = nfl;
    if (nfl > 0) {
        if (rq->last_n_keep > 0 && (!rq->last_lmk_index || !rq->last_lmk_col)) { h->err = "marginalize: previous prior landmark lists missing"; return SADVIO_E_INVALID_ARG; }
        if (rq->last_kf >= 0 && rq->last_kf_col < 0) { h->err = "marginalize: last_kf_col < 0"; return SADVIO_E_INVALID_ARG; }
        std::vector<int>& col = M.col;
        col.assign(nl, -1);
        if (rq->last_kf >= 0) {
            const int base = (rq->last_kf == rq->kf_marg) ? 0 : ((rq->last_kf == rq->kf_keep) ? kf_keep_col : -1);
            const int width = (rq->last_kf == rq->kf_marg) ? (rq->marg_has_imu ? 15 : 6) : 15;
            if (base >= 0) for (int a = 0; a < width && rq->last_kf_col + a < nl; a++) col[rq->last_kf_col + a] = base + a;
        }
        for (int k = 0; k < rq->last_n_keep; k++) {
            if (rq->last_lmk_col[k] < 0) continue;
            if (rq->last_lmk_col[k] + 3 > nl) { h->err = "marginalize: last_lmk_col exceeds the previous prior's columns"; return SADVIO_E_INVALID_ARG; }
            const int li = rq->last_lmk_index[k];
            if (li < 0 || li >= d.n_lmk) continue;
            const int lc = lcol[li];
            if (lc < 0) continue;
            for (int a = 0; a < 3; a++) col[rq->last_lmk_col[k] + a] = lc + a;
        }
    }
    return SADVIO_OK;
}

// 2. Allocate, ONE staged upload of the lists, then A = sum J^T J, b = sum J^T r over the blocks touching frame0
int marg_assemble(sadvio_ba_handle* h, const sadvio_marg_request* rq, const MargLayout& L, const MargRoutes& R) {
    MargScratch& M = h->mg;
    PriorState& PR = h->prior;
    const int m = L.m, n = L.n, N = L.N, nl = L.nl, nfl = L.nfl;
    SolveOpts so{};
    DevPtrs P = make_ptrs(h, so, 2);
    const int big = std::max(m, n + 1);
    HIP_TRY(M.A.alloc((size_t)N * N)); HIP_TRY(M.b.alloc(N)); HIP_TRY(M.flag.alloc(8));
    HIP_TRY(M.G.alloc((size_t)big * big)); HIP_TRY(M.V.alloc((size_t)big * big)); HIP_TRY(M.ev.alloc(big)); HIP_TRY(M.Vs.alloc((size_t)big * big));
    HIP_TRY(M.Ainv.alloc((size_t)m * m)); HIP_TRY(M.T.alloc((size_t)n * m)); HIP_TRY(M.Ak.alloc((size_t)n * n)); HIP_TRY(M.bk.alloc(n));
    HIP_TRY(M.newJ.alloc((size_t)n * n)); HIP_TRY(M.newr.alloc(n)); HIP_TRY(M.wtmp.alloc((size_t)big + 16));
    HIP_TRY(hipMemsetAsync(M.A.p, 0, sizeof(double) * (size_t)N * N, h->stream));
    HIP_TRY(hipMemsetAsync(M.b.p, 0, sizeof(double) * N, h->stream));
    const double* lastJ = PR.J.p; const double* lastr = PR.r0.p;   // (read where a previous prior exists)
    if (nfl > 0) {
        HIP_TRY(M.lastcol.alloc(nl));
        h->up.add(M.lastcol.p, M.col.data(), sizeof(int) * (size_t)nl);
        if (!L.last_resident) {
            HIP_TRY(M.lastJ.alloc((size_t)nfl * nl)); HIP_TRY(M.lastr.alloc(nfl));
            h->up.add(M.lastJ.p, rq->last_J, sizeof(double) * (size_t)nfl * nl);
            h->up.add(M.lastr.p, rq->last_r0, sizeof(double) * (size_t)nfl);
            lastJ = M.lastJ.p; lastr = M.lastr.p;
        }
    }
    const bool small = L.S.has_imu || L.S.n_prior;
    if (L.n_items > 0) { HIP_TRY(M.ditems.alloc(M.items.size())); h->up.add(M.ditems.p, M.items.data(), M.items.size() * sizeof(int)); }
    if (small) { HIP_TRY(M.small.alloc(1)); h->up.add(M.small.p, &L.S, sizeof(L.S)); }
    HIP_TRY(h->up.flush(h->stream));
    if (L.n_items > 0) {
        auto ko = h->plan.factor_type == SADVIO_FACTOR_PIXEL ? k_marg_obs<0> : k_marg_obs<1>;
        hipLaunchKernelGGL(ko, dim3((L.n_items + 127) / 128), dim3(128), 0, h->stream, P, M.ditems.p, L.n_items, M.A.p, M.b.p, N);
    }
    if (small) hipLaunchKernelGGL(k_marg_small, dim3(1), dim3(64), 0, h->stream, P, M.small.p, M.A.p, M.b.p, N);
    const dim3 grid_l((unsigned)(((long long)nl * nl + 255) / 256));
    switch (R.last) {
    case LastScatter::none: break;
    case LastScatter::resident_hg:
        hipLaunchKernelGGL(k_marg_last_scatter_h, grid_l, dim3(256), 0, h->stream, PR.H.p, PR.g.p, M.lastcol.p, nl, M.A.p, M.b.p, N);
        break;
    case LastScatter::gemm:
        HIP_TRY(M.Hl.alloc((size_t)nl * nl));
        launch_mgemm(h, M.Hl.p, nl, lastJ, 1LL, (long long)nl, lastJ, (long long)nl, 1LL, nl, nl, nfl, 1.0, 0.0);      // H = J^T J
        hipLaunchKernelGGL(k_marg_last_scatter, grid_l, dim3(256), 0, h->stream, M.Hl.p, lastJ, lastr, M.lastcol.p, nfl, nl, M.A.p, M.b.p, N);
        break;
    case LastScatter::small:
        hipLaunchKernelGGL(k_marg_last_prior, grid_l, dim3(256), 0, h->stream, lastJ, lastr, M.lastcol.p, nfl, nl, M.A.p, M.b.p, N);
        break;
    }
    return SADVIO_OK;
}

// The unpivoted attempt on a matrix expected to be positive definite (Amm, or Ak behind a full-rank prior): run_wfac on the copy in V
// (destroyed; A0, leading dimension ld0, is the original for the pivot test), y riding along. ok = every pivot is safely positive;
// then G holds the factor's rows like the pivoted route leaves them, y = L^-1 y and step_of the identity pivot order. Lx: n x n scratch.
int factor_unpivoted(sadvio_ba_handle* h, double* V, int n, double* y, double* Lx, const double* A0, long long ld0, double tau_rel, double* G, DevBuf<int>& step_of, bool& ok) {
    MargScratch& M = h->mg;
    ok = false;
    HIP_TRY(M.Vs.alloc(wfac_scratch_doubles(n)));   // (grow-only: the big x big of marg_assemble stays)
    double* Ltw = M.Vs.p; double* Ld = Ltw + (size_t)((n + WD - 1) / WD) * WD_LT;
    const int okf = run_wfac(h, V, n, y, Lx, Ltw, A0, ld0, tau_rel, M.wtmp.p, M.flag.p);
    if (okf < 0) { h->err = "marginalize: HIP error in the unpivoted Cholesky"; return SADVIO_E_HIP; }
    if (okf != 1) return SADVIO_OK;
    ok = true;
    hipLaunchKernelGGL(k_wfac_pack, dim3((unsigned)(((long long)n * n + 255) / 256)), dim3(256), 0, h->stream, Lx, (long long)n, Ltw, Ld, y, n, G, y);
    HIP_TRY(step_of.alloc(n));
    hipLaunchKernelGGL(k_iota, dim3((n + 255) / 256), dim3(256), 0, h->stream, step_of.p, n);
    return SADVIO_OK;
}

// Shared tail of the two Cholesky routes to Amm^-1: Vs = Z = G^-T of the factor in M.G / M.piv_mm, and the proof that no
// eigenvalue of Amm lies below the reference's cut (MargRoutes::mm_unpivoted). proven = false: NaN / inf included.
int mm_inverse_from_factor(sadvio_ba_handle* h, int m, int eig_cut_mode, bool& proven) {
    MargScratch& M = h->mg;
    const bool ref_cut = eig_cut_mode == SADVIO_EIG_CUT_REFERENCE;
    double trace = 0.0;
    if (int rc = prior_build_Z(h, M.G.p, m, m, SADVIO_PRIOR_FORM_CHOLESKY, M.piv_mm.p, M.Vs.p, eig_cut_mode, ref_cut ? &trace : nullptr)) return rc;
    proven = !ref_cut || trace < 1e12;
    return SADVIO_OK;
}

enum class MmRoute { wfac_cholesky, pivoted_cholesky, eigen };

// 3. Vs with Vs^T Vs = Amm^+: the unpivoted factor's inverse, else the pivoted factor's, else the eigen-decomposition under the
// request's cut. A factor that passes every pivot but fails the trace proof goes straight to the eigen-decomposition.
int marg_invert_mm(sadvio_ba_handle* h, const sadvio_marg_request* rq, const MargLayout& L, const MargRoutes& R, MmRoute& route, int& sweeps) {
    MargScratch& M = h->mg;
    const int m = L.m, N = L.N;
    const long long mm2 = (long long)m * m;
    const dim3 grid_mm((unsigned)((mm2 + 255) / 256));
    sweeps = 0;
    bool try_pivoted = R.mm_pivoted;
    if (R.mm_unpivoted) {
        bool ok = false, proven = false;
        hipLaunchKernelGGL(k_jacobi_init, grid_mm, dim3(256), 0, h->stream, M.A.p, (long long)N, m, M.V.p, M.G.p, 0);
        HIP_TRY(hipMemsetAsync(M.wtmp.p + 8, 0, sizeof(double) * (size_t)m, h->stream));
        if (int rc = factor_unpivoted(h, M.V.p, m, M.wtmp.p + 8, M.Ainv.p, M.A.p, (long long)N, pchol_tau(m, SADVIO_EIG_CUT_REFERENCE), M.G.p, M.piv_mm, ok)) return rc;
        if (ok) {
            if (int rc = mm_inverse_from_factor(h, m, rq->eig_cut_mode, proven)) return rc;
            if (proven) { route = MmRoute::wfac_cholesky; return SADVIO_OK; }
            try_pivoted = false;
        }
    }
    if (try_pivoted) {
        bool proven = false;
        hipLaunchKernelGGL(k_jacobi_init, grid_mm, dim3(256), 0, h->stream, M.A.p, (long long)N, m, M.V.p, M.G.p, 0);
        const int r = run_pchol(h, M.V.p, m, M.G.p, pchol_tau(m, SADVIO_EIG_CUT_NOISE_FLOOR));
        if (r < 0) { h->err = "marginalize: HIP error in the pivoted Cholesky"; return SADVIO_E_HIP; }
        if (r == m) {
            HIP_TRY(M.piv_mm.alloc(m));
            HIP_TRY(hipMemcpyAsync(M.piv_mm.p, h->d_jac_ints.p, sizeof(int) * (size_t)m, hipMemcpyDeviceToDevice, h->stream));
            if (int rc = mm_inverse_from_factor(h, m, rq->eig_cut_mode, proven)) return rc;
            if (proven) { route = MmRoute::pivoted_cholesky; return SADVIO_OK; }
        }
    }
    route = MmRoute::eigen;
    sweeps = run_jacobi(h, M.A.p, N, m, 0, M.G.p, M.V.p, M.ev.p, M.flag.p, rq->eig_cut_mode);
    if (sweeps < 0) { h->err = "marginalize: HIP error in the eigen-solver"; return SADVIO_E_HIP; }
    std::vector<double>& hev = M.hev;
    hev.resize(m);
    HIP_TRY(hipMemcpyAsync(hev.data(), M.ev.p, sizeof(double) * m, hipMemcpyDeviceToHost, h->stream));
    HIP_TRY(hipStreamSynchronize(h->stream));
    const double cut = marg_cut(hev, rq->eig_cut_mode);
    std::vector<double>& sel = M.hsel;   // (kept in the handle: the upload below is asynchronous; marg_schur waits for it)
    sel.resize(m);
    for (int i = 0; i < m; i++) sel[i] = hev[i] > cut ? 1.0 / sqrt(hev[i]) : 0.0;
    HIP_TRY(hipMemcpyAsync(M.ev.p, sel.data(), sizeof(double) * m, hipMemcpyHostToDevice, h->stream));
    hipLaunchKernelGGL(k_scale_rows, grid_mm, dim3(256), 0, h->stream, M.V.p, M.ev.p, m, M.Vs.p);
    return SADVIO_OK;
}

// 4. Ainv = Vs^T Vs (Vs = Lambda^-1/2 U^T, or Z = G^-T of the Cholesky routes) ; T = Arm Ainv ; Ak = Arr - T Arm^T ; bk = brr - T bmm   (FP64 matrix cores)
int marg_schur(sadvio_ba_handle* h, const MargLayout& L, MmRoute route) {
    MargScratch& M = h->mg;
    const int m = L.m, n = L.n, N = L.N;
    launch_mgemm(h, M.Ainv.p, m, M.Vs.p, 1LL, (long long)m, M.Vs.p, (long long)m, 1LL, m, m, m, 1.0, 0.0);
    launch_mgemm(h, M.T.p, m, M.A.p + (size_t)m * N, (long long)N, 1LL, M.Ainv.p, (long long)m, 1LL, n, m, m, 1.0, 0.0);
    HIP_TRY(hipMemcpy2DAsync(M.Ak.p, sizeof(double) * n, M.A.p + (size_t)m * N + m, sizeof(double) * N, sizeof(double) * n, n, hipMemcpyDeviceToDevice, h->stream));
    launch_mgemm(h, M.Ak.p, n, M.T.p, (long long)m, 1LL, M.A.p + (size_t)m * N, 1LL, (long long)N, n, n, m, -1.0, 1.0);
    hipLaunchKernelGGL(k_marg_bk, dim3((n + 127) / 128), dim3(128), 0, h->stream, M.T.p, M.b.p, n, m, M.bk.p);
    if (route == MmRoute::eigen) HIP_TRY(hipStreamSynchronize(h->stream));   // before a later call can overwrite M.hsel, whose upload the eigen route queued
    return SADVIO_OK;
}

// 5a. Cholesky form: J = G with G^T G = Ak (rank-revealing, pivots cut like the eigenvalues), r0 = -G^-T bk as the
// factor's extra column. No eigen-decomposition. hg = the new prior is of full rank by the unpivoted route: it may keep Ak, bk.
int marg_factor_cholesky(sadvio_ba_handle* h, const sadvio_marg_request* rq, const MargLayout& L, const MargRoutes& R, int& nf, bool& hg) {
    MargScratch& M = h->mg;
    PriorState& PR = h->prior;
    const int n = L.n, n1 = n + 1;
    const long long nn1 = (long long)n1 * n1;
    h->marg_stats[0]++;
    hg = false;
    if (R.k_unpivoted) {
        // A prior that carries an earlier prior is normally of full rank: then the factor needs no pivoting and the wide-panel
        // solver of the dense reduced systems (dense_chol.h: k_wchol_diag16 + k_wchol_step, one launch per 96 columns, bk riding
        // along as its right-hand side) delivers L and z = L^-1 bk in a third of the pivoted factorisation's time. Every pivot is
        // tested afterwards (k_wfac_diag); one that is not safely positive sends the call to the rank-revealing route below.
        HIP_TRY(hipMemcpyAsync(M.V.p, M.Ak.p, sizeof(double) * (size_t)n * n, hipMemcpyDeviceToDevice, h->stream));
        HIP_TRY(hipMemcpyAsync(M.newr.p, M.bk.p, sizeof(double) * (size_t)n, hipMemcpyDeviceToDevice, h->stream));
        if (int rc = factor_unpivoted(h, M.V.p, n, M.newr.p, M.G.p, M.Ak.p, (long long)n, pchol_tau(n, rq->eig_cut_mode), M.newJ.p, PR.step_of, hg)) return rc;
        h->marg_stats[hg ? 1 : 2]++;
        if (hg) { nf = n; return SADVIO_OK; }
    }
    hipLaunchKernelGGL(k_marg_aug_init, dim3((unsigned)((nn1 + 255) / 256)), dim3(256), 0, h->stream, M.Ak.p, M.bk.p, n, M.V.p);
    nf = run_pchol(h, M.V.p, n1, M.G.p, pchol_tau(n, rq->eig_cut_mode));
    if (nf < 0) { h->err = "marginalize: HIP error in the pivoted Cholesky"; return SADVIO_E_HIP; }
    if (nf > n) nf = n;
    if (rq->eig_cut_mode == SADVIO_EIG_CUT_REFERENCE && nf > 0) {
        const int rc = refine_rank_by_eigenvalue(h, M.G.p, n1, nf);
        if (rc < 0) { h->err = "marginalize: HIP error in the rank refinement"; return SADVIO_E_HIP; }
        nf = rc;
    }
    if (nf > 0) {
        const long long cnt = (long long)nf * n1;
        hipLaunchKernelGGL(k_marg_pack_chol, dim3((unsigned)((cnt + 255) / 256)), dim3(256), 0, h->stream, M.G.p, n, h->d_jac_ints.p + n1, M.newJ.p, M.newr.p);
        HIP_TRY(PR.step_of.alloc(n));
        HIP_TRY(hipMemcpyAsync(PR.step_of.p, h->d_jac_ints.p, sizeof(int) * (size_t)n, hipMemcpyDeviceToDevice, h->stream));
    }
    return SADVIO_OK;
}

// 5b. Eigen form: rank-revealing decomposition of Ak (lower triangle, as Eigen reads it), marginalization.cpp:318-342
int marg_factor_eigen(sadvio_ba_handle* h, const sadvio_marg_request* rq, const MargLayout& L, int& nf, int& sweeps) {
    MargScratch& M = h->mg;
    const int n = L.n;
    sweeps = run_jacobi(h, M.Ak.p, n, n, 1, M.G.p, M.V.p, M.ev.p, M.flag.p, rq->eig_cut_mode);
    if (sweeps < 0) { h->err = "marginalize: HIP error in the eigen-solver"; return SADVIO_E_HIP; }
    std::vector<double>& hev = M.hev;
    hev.resize(n);
    HIP_TRY(hipMemcpyAsync(hev.data(), M.ev.p, sizeof(double) * n, hipMemcpyDeviceToHost, h->stream));
    HIP_TRY(hipStreamSynchronize(h->stream));
    const double cut = marg_cut(hev, rq->eig_cut_mode);
    // ascending eigenvalue order, like Eigen::SelfAdjointEigenSolver (row order of J only)
    std::vector<int> order(n), sel_rows;
    for (int i = 0; i < n; i++) order[i] = i;
    std::sort(order.begin(), order.end(), [&](int a, int b) { return hev[a] < hev[b]; });
    for (int i : order) if (hev[i] > cut) sel_rows.push_back(i);
    nf = (int)sel_rows.size();
    if (nf > 0) {
        HIP_TRY(M.sel.alloc(nf));
        HIP_TRY(hipMemcpyAsync(M.sel.p, sel_rows.data(), sizeof(int) * nf, hipMemcpyHostToDevice, h->stream));
        hipLaunchKernelGGL(k_marg_prior, dim3(nf), dim3(JAC_THREADS), 0, h->stream, M.V.p, M.ev.p, M.sel.p, nf, n, M.bk.p, M.newJ.p, M.newr.p);
        HIP_TRY(hipStreamSynchronize(h->stream));   // sel_rows goes out of scope
    }
    return SADVIO_OK;
}

// 6. The new prior becomes the handle's (AOptimizer.h:88-90: _marginalization_last), the old one's buffers become scratch
int marg_install(sadvio_ba_handle* h, const sadvio_marg_request* rq, const MargLayout& L, bool chol_form, int nf, bool hg, double* J_out, double* r0_out) {
    MargScratch& M = h->mg;
    PriorState& PR = h->prior;
    const int n = L.n;
    PR.J.swap(M.newJ); PR.r0.swap(M.newr);
    PR.serial++;
    PR.hg_valid = false;
    if (hg) { PR.H.swap(M.Ak); PR.g.swap(M.bk); PR.hg_valid = true; }   // (full rank: J^T J = Ak, J^T r0 = -bk to rounding)
    PR.valid = nf > 0; PR.z_valid = false; PR.n_full = nf; PR.n = n; PR.form = chol_form ? SADVIO_PRIOR_FORM_CHOLESKY : SADVIO_PRIOR_FORM_EIGEN; PR.cut_mode = rq->eig_cut_mode;
    if (nf > 0) {
        if (J_out) HIP_TRY(hipMemcpyAsync(J_out, PR.J.p, sizeof(double) * (size_t)nf * n, hipMemcpyDeviceToHost, h->stream));
        if (r0_out) HIP_TRY(hipMemcpyAsync(r0_out, PR.r0.p, sizeof(double) * nf, hipMemcpyDeviceToHost, h->stream));
    }
    // the prior stays on the device and everything that reads it is stream-ordered behind this call: only a read-back has to wait
    // (asynchronous contract, sadvio_ba.h: a fault of the tail kernels surfaces in the next call that waits on this handle's stream;
    // SADVIO_DEBUG != 0 or cfg.profile_kernels wait here so that it is attributed to marginalize)
    if ((nf > 0 && (J_out || r0_out)) || h->env.debug || h->cfg.profile_kernels) HIP_TRY(hipStreamSynchronize(h->stream));
    HIP_TRY(hipGetLastError());
    return SADVIO_OK;
}

// sadvio_ba_marginalize behind its argument checks: BundleAdjustmentCERESAnalytic::marginalize (…Analytic.cpp:431-663) on the device
int marginalize(sadvio_ba_handle* h, int w, const sadvio_marg_request* rq, sadvio_marg_result* res, int32_t* lmk_col_out, double* J_out, double* r0_out) {
    MargLayout L;
    if (int rc = marg_layout(h, w, rq, L, res, lmk_col_out)) return rc;
    const MargRoutes R = marg_routes(h, rq, L);
    if (int rc = marg_assemble(h, rq, L, R)) return rc;
    MmRoute mm_route;
    int sweeps_mm = 0, sweeps_k = 0, nf = 0;
    if (int rc = marg_invert_mm(h, rq, L, R, mm_route, sweeps_mm)) return rc;
    if (res) res->sweeps_mm = sweeps_mm;
    if (int rc = marg_schur(h, L, mm_route)) return rc;
    bool hg = false;   // the new prior keeps Ak, bk (full rank by the unpivoted route)
    if (int rc = R.chol_form ? marg_factor_cholesky(h, rq, L, R, nf, hg) : marg_factor_eigen(h, rq, L, nf, sweeps_k)) return rc;
    if (res) { res->sweeps_k = sweeps_k; res->n_full = nf; }
    return marg_install(h, rq, L, R.chol_form, nf, hg, J_out, r0_out);
}

// host-side post-processing of the tiny (3x3 / 15x15) NFR covariances
void host_sym_eig(const double* Ain, int n, double* ev, double* V) {
    double A[225];
    memcpy(A, Ain, sizeof(double) * n * n);
    for (int i = 0; i < n; i++) for (int j = 0; j < n; j++) V[i * n + j] = i == j ? 1.0 : 0.0;
    for (int sweep = 0; sweep < 100; sweep++) {
        double off = 0, diag = 0;
        for (int i = 0; i < n; i++) { diag += A[i * n + i] * A[i * n + i]; for (int j = i + 1; j < n; j++) off += A[i * n + j] * A[i * n + j]; }
        if (off <= 1e-60 || off <= 1e-32 * diag) break;
        for (int p = 0; p < n - 1; p++)
            for (int q = p + 1; q < n; q++) {
                const double apq = A[p * n + q];
                if (apq == 0.0) continue;
                const double theta = (A[q * n + q] - A[p * n + p]) / (2.0 * apq);
                const double t = (theta >= 0 ? 1.0 : -1.0) / (std::fabs(theta) + std::sqrt(theta * theta + 1.0));
                const double c = 1.0 / std::sqrt(t * t + 1.0), s = t * c;
                for (int k = 0; k < n; k++) { const double a = A[k * n + p], b = A[k * n + q]; A[k * n + p] = c * a - s * b; A[k * n + q] = s * a + c * b; }
                for (int k = 0; k < n; k++) { const double a = A[p * n + k], b = A[q * n + k]; A[p * n + k] = c * a - s * b; A[q * n + k] = s * a + c * b; }
                for (int k = 0; k < n; k++) { const double a = V[k * n + p], b = V[k * n + q]; V[k * n + p] = c * a - s * b; V[k * n + q] = s * a + c * b; }
            }
    }
    for (int i = 0; i < n; i++) ev[i] = A[i * n + i];
}

bool host_inverse(const double* A, int n, double* Ai) {
    std::vector<double> M((size_t)n * 2 * n);
    for (int i = 0; i < n; i++) for (int j = 0; j < n; j++) { M[i * 2 * n + j] = A[i * n + j]; M[i * 2 * n + n + j] = i == j ? 1.0 : 0.0; }
    for (int c = 0; c < n; c++) {
        int p = c;
        for (int r = c + 1; r < n; r++) if (std::fabs(M[r * 2 * n + c]) > std::fabs(M[p * 2 * n + c])) p = r;
        if (M[p * 2 * n + c] == 0.0) return false;
        if (p != c) for (int j = 0; j < 2 * n; j++) std::swap(M[c * 2 * n + j], M[p * 2 * n + j]);
        const double d = 1.0 / M[c * 2 * n + c];
        for (int j = 0; j < 2 * n; j++) M[c * 2 * n + j] *= d;
        for (int r = 0; r < n; r++) {
            if (r == c) continue;
            const double f = M[r * 2 * n + c];
            if (f != 0.0) for (int j = 0; j < 2 * n; j++) M[r * 2 * n + j] -= f * M[c * 2 * n + j];
        }
    }
    for (int i = 0; i < n; i++) for (int j = 0; j < n; j++) Ai[i * n + j] = M[i * 2 * n + n + j];
    return true;
}

// symmetric square root of the information of an NFR factor from its covariance (marginalization.cpp:379-385 /
// :482-487): VIO inverts first and keeps eigenvalues > 1e-12, VO inverts the eigenvalues > 1e-12
bool nfr_sqrt_info(const double* S, int rows, bool invert_first, double* W) {
    double M[225], ev[15], V[225];
    if (invert_first) { if (!host_inverse(S, rows, M)) return false; }
    else memcpy(M, S, sizeof(double) * rows * rows);
    for (int i = 0; i < rows; i++) for (int j = 0; j < i; j++) { const double s = 0.5 * (M[i * rows + j] + M[j * rows + i]); M[i * rows + j] = M[j * rows + i] = s; }
    host_sym_eig(M, rows, ev, V);
    for (int i = 0; i < rows; i++)
        for (int j = 0; j < rows; j++) {
            double s = 0;
            for (int k = 0; k < rows; k++) {
                const double e = ev[k] > 1e-12 ? (invert_first ? ev[k] : 1.0 / ev[k]) : 0.0;
                s += V[i * rows + k] * std::sqrt(e) * V[j * rows + k];
            }
            W[i * rows + j] = s;
        }
    return true;
}

// sadvio_ba_marginalize_relative behind its argument checks
int marginalize_relative(sadvio_ba_handle* h, int w, int kf_a, int kf_b, int eig_cut_mode, double* inf36, double* Ak144) {
    const WinDev& d = h->plan.wins[w].d;
    HIP_TRY(hipSetDevice(h->device));
    // preMarginalizeRelative (marginalization.cpp:532-588): a landmark of frame a is entered once per feature it has in frame b
    const int ga = d.kf_base + kf_a, gb = d.kf_base + kf_b;
    std::vector<int> items;
    int m = 0;
    for (int l = 0; l < d.n_lmk; l++) {
        const int gl = d.lmk_base + l;
        int ca = 0, cb = 0;
        const int ob = h->plan.lmk_ob[gl], oe = h->plan.lmk_oe[gl];
        auto count = [&](int lo, int hi) {
            for (int o = lo; o < hi; o++) {
                if (h->plan.obs_perm[o] < 0) continue;      // pseudo-observation of a sparse prior factor
                ca += h->plan.obs_kf[o] == ga; cb += h->plan.obs_kf[o] == gb;
            }
        };
        if (oe - ob > MAX_LMK_OBS) {   // a long track: the runs of the two key-frames alone (rel_runs.h)
            const RelRuns rr = rel_runs(h->plan.obs_kf.data(), ob, oe, ga, gb);
            count(rr.lo[0], rr.hi[0]); count(rr.lo[1], rr.hi[1]);
        } else count(ob, oe);
        if (ca > 0 && cb > 0) { items.push_back(gl); items.push_back(cb); m += 3 * cb; }
    }
    const int n_items = (int)items.size() / 2;
    if (n_items == 0) { h->err = "marginalize_relative: the two key-frames share no landmark"; return SADVIO_E_REFUSED; }
    DevBuf<int> ditems; DevBuf<double> dscr, dAk, dJ; DevBuf<unsigned long long> dmax;
    HIP_TRY(ditems.alloc(items.size())); HIP_TRY(dscr.alloc((size_t)n_items * RELM_ROW)); HIP_TRY(dAk.alloc(144)); HIP_TRY(dJ.alloc(72)); HIP_TRY(dmax.alloc(1));
    HIP_TRY(hipMemcpyAsync(ditems.p, items.data(), items.size() * sizeof(int), hipMemcpyHostToDevice, h->stream));
    HIP_TRY(hipMemsetAsync(dAk.p, 0, 144 * sizeof(double), h->stream)); HIP_TRY(hipMemsetAsync(dmax.p, 0, 8, h->stream));
    SolveOpts o{};
    DevPtrs P = make_ptrs(h, o, 1);
    auto kl = h->plan.factor_type == SADVIO_FACTOR_PIXEL ? k_relmarg_lmk<0> : k_relmarg_lmk<1>;
    hipLaunchKernelGGL(kl, dim3((n_items + 63) / 64), dim3(64), 0, h->stream, P, ditems.p, n_items, ga, gb, dscr.p, dAk.p, dmax.p);
    hipLaunchKernelGGL(k_relmarg_apply, dim3((n_items + 63) / 64), dim3(64), 0, h->stream, dscr.p, n_items, m, dmax.p, dAk.p, eig_cut_mode == SADVIO_EIG_CUT_NOISE_FLOOR ? 1 : 0);
    hipLaunchKernelGGL(k_relmarg_jac, dim3(1), dim3(64), 0, h->stream, P, ga, gb, dJ.p);
    HIP_TRY(hipGetLastError());
    double Ak[144], J[72];
    HIP_TRY(hipMemcpyAsync(Ak, dAk.p, sizeof(Ak), hipMemcpyDeviceToHost, h->stream));
    HIP_TRY(hipMemcpyAsync(J, dJ.p, sizeof(J), hipMemcpyDeviceToHost, h->stream));
    HIP_TRY(hipStreamSynchronize(h->stream));
    if (Ak144) memcpy(Ak144, Ak, sizeof(Ak));
    // rankReveallingDecomposition (Eigen reads the lower triangle) -> Sigma_k = U diag(1 / lambda) U^T (marginalization.cpp:255-262)
    double As[144], ev[12], V[144], Sk[144];
    for (int i = 0; i < 12; i++) for (int j = 0; j <= i; j++) As[12 * i + j] = As[12 * j + i] = Ak[12 * i + j];
    host_sym_eig(As, 12, ev, V);
    double mx = 0.0;
    for (int k = 0; k < 12; k++) mx = std::max(mx, std::fabs(ev[k]));
    // SADVIO_EIG_CUT_NOISE_FLOOR: the floor of the Schur complement = a sum over the marginalised landmarks (see oracle/marg.c):
    // the gauge null space of Ak computes to ~ eps * lambda_max * n_items; SADVIO_EIG_CUT_REFERENCE: the reference's absolute 1e-12
    const double cut = eig_cut_mode == SADVIO_EIG_CUT_NOISE_FLOOR ? std::max(1e-12, 12 * 2.220446049250313e-16 * mx * (2.0 + n_items)) : 1e-12;
    memset(Sk, 0, sizeof(Sk));
    for (int k = 0; k < 12; k++) {
        if (!(ev[k] > cut)) continue;
        const double iv = 1.0 / ev[k];
        for (int i = 0; i < 12; i++) for (int j = 0; j < 12; j++) Sk[12 * i + j] += V[12 * i + k] * iv * V[12 * j + k];
    }
    double JS[72], cov[36];
    for (int i = 0; i < 6; i++) for (int j = 0; j < 12; j++) { double s2 = 0; for (int k = 0; k < 12; k++) s2 += J[12 * i + k] * Sk[12 * k + j]; JS[12 * i + j] = s2; }
    for (int i = 0; i < 6; i++) for (int j = 0; j < 6; j++) { double s2 = 0; for (int k = 0; k < 12; k++) s2 += JS[12 * i + k] * J[12 * j + k]; cov[6 * i + j] = s2; }
    if (!host_inverse(cov, 6, inf36)) { h->err = "marginalize_relative: singular covariance of the relative pose"; return SADVIO_E_REFUSED; }
    return SADVIO_OK;
}

// The prior's rows and Z with Z^T Z = Sigma_k on the device: the handle's prior (J = NULL; its Z is built by the first sparsify of it)
// or the caller's rows, in eigen form
int sparsify_prior_on_device(sadvio_ba_handle* h, const double* J, int nf, int n, const double*& dJ, const double*& dZ) {
    PriorState& PR = h->prior;
    MargScratch& M = h->mg;
    if (!J) {
        dJ = PR.J.p;
        if (!PR.z_valid) {
            HIP_TRY(PR.Z.alloc((size_t)nf * n));
            const int rc = prior_build_Z(h, PR.J.p, nf, n, PR.form, PR.step_of.p, PR.Z.p, PR.cut_mode, nullptr, true);   // guard: Sigma_k = the pseudo-inverse the reference takes (marginalization.cpp:255-262)
            if (rc != SADVIO_OK) return rc;
            PR.z_valid = true;
        }
        dZ = PR.Z.p;
    } else {
        HIP_TRY(M.lastJ.alloc((size_t)nf * n)); HIP_TRY(M.Zt.alloc((size_t)nf * n));
        HIP_TRY(hipMemcpyAsync(M.lastJ.p, J, sizeof(double) * (size_t)nf * n, hipMemcpyHostToDevice, h->stream));
        const int rc = prior_build_Z(h, M.lastJ.p, nf, n, SADVIO_PRIOR_FORM_EIGEN, nullptr, M.Zt.p, SADVIO_EIG_CUT_REFERENCE);
        if (rc != SADVIO_OK) return rc;
        dJ = M.lastJ.p; dZ = M.Zt.p;
    }
    return SADVIO_OK;
}

// sadvio_ba_sparsify behind its argument checks: Marginalization::sparsifyVIO / sparsifyVO (marginalization.cpp:362-514)
int sparsify(sadvio_ba_handle* h, int w, int vio, int nf, int n, const double* J, int kf_keep, int kf_col, int n_keep, const int32_t* lmk_index, const int32_t* lmk_col,
             int32_t* n_out, sadvio_sparse_prior* out) {
    PriorState& PR = h->prior;
    MargScratch& M = h->mg;
    if (!J) {   // the handle's prior
        if (!PR.valid) { h->err = "sparsify: J = NULL but the handle holds no prior"; return SADVIO_E_STATE; }
        nf = PR.n_full; n = PR.n;
    }
    if (n <= 0 || nf <= 0) { h->err = "sparsify: empty prior"; return SADVIO_E_REFUSED; }
    const HostWin& HW = h->plan.wins[w];
    const WinDev& d = HW.d;
    const SrcWin& SW = h->src[w];
    if (vio && (kf_keep < 0 || kf_keep >= d.n_kf || kf_col < 0 || kf_col + 15 > n)) { h->err = "sparsify: kept key-frame out of range"; return SADVIO_E_INVALID_ARG; }
    for (int k = 0; k < n_keep; k++)
        if (lmk_col[k] >= 0 && (lmk_index[k] < 0 || lmk_index[k] >= d.n_lmk || lmk_col[k] + 3 > n)) { h->err = "sparsify: kept landmark out of range"; return SADVIO_E_INVALID_ARG; }
    HIP_TRY(hipSetDevice(h->device));
    // linearisation values of the window: the handle's deep copy of the caller's arrays (no read-back)
    double T[12], v3[3] = {0, 0, 0}, ba3[3] = {0, 0, 0}, bg3[3] = {0, 0, 0};
    if (vio) {
        memcpy(T, &SW.kf_T[12 * (size_t)kf_keep], sizeof(T));
        if (!SW.kf_vel.empty()) memcpy(v3, &SW.kf_vel[3 * (size_t)kf_keep], 24);
        if (!SW.kf_ba.empty()) memcpy(ba3, &SW.kf_ba[3 * (size_t)kf_keep], 24);
        if (!SW.kf_bg.empty()) memcpy(bg3, &SW.kf_bg[3 * (size_t)kf_keep], 24);
    }
    const double* lp = SW.lmk_p.data();
    const double* dJ = nullptr; const double* dZ = nullptr;
    if (int rc = sparsify_prior_on_device(h, J, nf, n, dJ, dZ)) return rc;
    std::vector<NfrSpecC> specs;
    std::vector<double> jsel(4 * 225, 0.0);
    std::vector<int> kept;  // positions k with lmk_col >= 0
    for (int k = 0; k < n_keep; k++) if (lmk_col[k] >= 0) kept.push_back(k);
    std::vector<int> order;  // VO: chain order (indices into kept)
    int out_off = 0;
    auto push = [&](int rows, int cols, int js) { NfrSpecC s{}; s.rows = rows; s.cols = cols; s.jsel = js; s.out_off = out_off; out_off += rows * rows; specs.push_back(s); return &specs.back(); };
    if (vio) {
        double tsk[9] = {0, -T[11], T[10], T[11], 0, -T[9], -T[10], T[9], 0}, Rt[9];
        for (int i = 0; i < 3; i++) for (int j = 0; j < 3; j++) { double s = 0; for (int k = 0; k < 3; k++) s += T[3 * i + k] * tsk[3 * k + j]; Rt[3 * i + j] = s; }
        double* J0 = &jsel[0];       // IMUPriordx selector 15 x 15 (marginalization.cpp:366-378)
        for (int a = 0; a < 15; a++) J0[a * 15 + a] = 1.0;
        for (int i = 0; i < 3; i++) for (int j = 0; j < 3; j++) { J0[i * 15 + j] = T[3 * i + j]; J0[i * 15 + 3 + j] = T[3 * i + j]; J0[(3 + i) * 15 + 3 + j] = T[3 * i + j]; }
        double* J1 = &jsel[225];     // PoseToLandmarkFactor selector 3 x 9: [R | -R [t]x | R] on (landmark, rotation, translation)
        for (int i = 0; i < 3; i++) for (int j = 0; j < 3; j++) { J1[i * 9 + j] = T[3 * i + j]; J1[i * 9 + 3 + j] = -Rt[3 * i + j]; J1[i * 9 + 6 + j] = T[3 * i + j]; }
        NfrSpecC* f = push(15, 15, 0);
        for (int a = 0; a < 15; a++) f->cidx[a] = kf_col + a;
        for (int k : kept) {
            NfrSpecC* s = push(3, 9, 1);
            s->fin = 1;   // the kernel returns the factor's information square root (nfr_sqrt_info3), not its covariance
            for (int a = 0; a < 3; a++) { s->cidx[a] = lmk_col[k] + a; s->cidx[3 + a] = kf_col + a; s->cidx[6 + a] = kf_col + 3 + a; }
        }
    } else {
        const int K = (int)kept.size();
        if (K < 2) { h->err = "sparsify: fewer than two kept landmarks"; return SADVIO_E_REFUSED; }
        std::vector<int> lc(K);
        for (int a = 0; a < K; a++) lc[a] = lmk_col[kept[a]];
        HIP_TRY(M.lc.alloc(K)); HIP_TRY(M.mi.alloc((size_t)K * K));
        HIP_TRY(hipMemcpyAsync(M.lc.p, lc.data(), sizeof(int) * K, hipMemcpyHostToDevice, h->stream));
        HIP_TRY(hipMemsetAsync(M.mi.p, 0, sizeof(double) * (size_t)K * K, h->stream));
        hipLaunchKernelGGL(k_nfr_trace, dim3((K * K + 255) / 256), dim3(256), 0, h->stream, dJ, nf, n, M.lc.p, K, M.mi.p);
        std::vector<double> mi((size_t)K * K);
        HIP_TRY(hipMemcpyAsync(mi.data(), M.mi.p, sizeof(double) * (size_t)K * K, hipMemcpyDeviceToHost, h->stream));
        HIP_TRY(hipStreamSynchronize(h->stream));
        // greedy chain (marginalization.cpp:432-456); Eigen's maxCoeff visits a column-major matrix column by column
        int mr = 0, mc = 0; double best = -1;
        for (int j = 0; j < K; j++) for (int i = 0; i < K; i++) if (mi[(size_t)i * K + j] > best) { best = mi[(size_t)i * K + j]; mr = i; mc = j; }
        order.push_back(mr); order.push_back(mc);
        for (int i = 0; i < K; i++) { mi[(size_t)i * K + mr] = 0; mi[(size_t)mr * K + i] = 0; mi[(size_t)i * K + mc] = 0; }
        int cur = mc;
        for (;;) {
            int bc = 0; double bv = mi[(size_t)cur * K];
            for (int j = 1; j < K; j++) if (mi[(size_t)cur * K + j] > bv) { bv = mi[(size_t)cur * K + j]; bc = j; }
            if (bv == 0) break;
            order.push_back(bc);
            for (int j = 0; j < K; j++) mi[(size_t)cur * K + j] = 0;
            for (int i = 0; i < K; i++) mi[(size_t)i * K + bc] = 0;
            cur = bc;
        }
        double* J2 = &jsel[2 * 225];   // identity 3 x 3
        double* J3 = &jsel[3 * 225];   // [I -I] 3 x 6
        for (int q = 0; q < 3; q++) { J2[q * 3 + q] = 1.0; J3[q * 6 + q] = 1.0; J3[q * 6 + 3 + q] = -1.0; }
        // covariance of every ordered landmark (entropy root, unary factor) then of every chain link
        for (int a : order) {
            NfrSpecC* s = push(3, 3, 2);
            for (int q = 0; q < 3; q++) s->cidx[q] = lmk_col[kept[a]] + q;
        }
        for (size_t k = 0; k + 1 < order.size(); k++) {
            NfrSpecC* s = push(3, 6, 3);
            for (int q = 0; q < 3; q++) { s->cidx[q] = lmk_col[kept[order[k]]] + q; s->cidx[3 + q] = lmk_col[kept[order[k + 1]]] + q; }
        }
    }
    const int ns = (int)specs.size();
    HIP_TRY(M.spec.alloc(ns)); HIP_TRY(M.jsel.alloc(4 * 225)); HIP_TRY(M.S.alloc((size_t)std::max(out_off, 1)));
    h->up.add(M.spec.p, specs.data(), sizeof(NfrSpecC) * (size_t)ns);
    h->up.add(M.jsel.p, jsel.data(), sizeof(double) * jsel.size());
    HIP_TRY(h->up.flush(h->stream));
    int first3 = 0;
    if (vio) {
        // the one 15-row factor (IMUPriordx) as two matrix-core products — W = Jsel Z[:, kf]^T (15 x nf), cov = W W^T — instead of
        // 120 LDS atomics per row of Z from one workgroup (measured 1.0 ms of the 1.6 ms call)
        HIP_TRY(M.T.alloc((size_t)15 * nf));
        launch_mgemm(h, M.T.p, nf, M.jsel.p, 15LL, 1LL, dZ + kf_col, 1LL, (long long)n, 15, nf, 15, 1.0, 0.0);
        launch_mgemm(h, M.S.p + specs[0].out_off, 15, M.T.p, (long long)nf, 1LL, M.T.p, 1LL, (long long)nf, 15, 15, nf, 1.0, 0.0);
        first3 = 1;
    }
    if (ns > first3) hipLaunchKernelGGL(k_nfr_cov_z, dim3(ns - first3), dim3(JAC_THREADS), 0, h->stream, dZ, nf, n, M.spec.p + first3, M.jsel.p, M.S.p);
    std::vector<double>& S = M.hS;
    S.resize((size_t)out_off);
    HIP_TRY(hipMemcpyAsync(S.data(), M.S.p, sizeof(double) * (size_t)out_off, hipMemcpyDeviceToHost, h->stream));
    HIP_TRY(hipStreamSynchronize(h->stream));
    HIP_TRY(hipGetLastError());
    int cnt = 0;
    auto fail = [&]() { h->err = "sparsify: singular factor covariance"; return SADVIO_E_NOT_USABLE; };
    if (vio) {
        sadvio_sparse_prior* o = out + cnt++;
        memset(o, 0, sizeof(*o));
        o->type = SADVIO_SPARSE_IMU_PRIOR; o->kf = kf_keep; o->lmk0 = o->lmk1 = -1;
        memcpy(o->T_prior, T, sizeof(T)); memcpy(o->v_prior, v3, 24); memcpy(o->ba_prior, ba3, 24); memcpy(o->bg_prior, bg3, 24);
        if (!nfr_sqrt_info(&S[specs[0].out_off], 15, true, o->sqrt_inf)) return fail();
        for (size_t i = 0; i < kept.size(); i++) {
            const int k = kept[i];
            o = out + cnt++;
            memset(o, 0, sizeof(*o));
            o->type = SADVIO_SPARSE_POSE_TO_LMK; o->kf = kf_keep; o->lmk0 = lmk_index[k]; o->lmk1 = -1;
            const double* p = &lp[3 * (size_t)lmk_index[k]];
            for (int a = 0; a < 3; a++) o->delta[a] = T[3 * a] * p[0] + T[3 * a + 1] * p[1] + T[3 * a + 2] * p[2] + T[9 + a];
            const double* Wd = &S[specs[i + 1].out_off];    // taken on the device
            for (int a = 0; a < 9; a++) { if (!std::isfinite(Wd[a])) return fail(); o->sqrt_inf[a] = Wd[a]; }
        }
    } else {
        const int no = (int)order.size();
        int root = 0; double best_det = 0;
        for (int k = 0; k < no; k++) {
            const double* s = &S[specs[k].out_off];
            const double det = s[0] * (s[4] * s[8] - s[5] * s[7]) - s[1] * (s[3] * s[8] - s[5] * s[6]) + s[2] * (s[3] * s[7] - s[4] * s[6]);
            if (k == 0 || det < best_det) { best_det = det; root = k; }
        }
        sadvio_sparse_prior* o = out + cnt++;
        memset(o, 0, sizeof(*o));
        const int lr = lmk_index[kept[order[root]]];
        o->type = SADVIO_SPARSE_LMK_PRIOR; o->kf = -1; o->lmk0 = lr; o->lmk1 = -1;
        memcpy(o->delta, &lp[3 * (size_t)lr], 24);
        if (!nfr_sqrt_info(&S[specs[root].out_off], 3, false, o->sqrt_inf)) return fail();
        for (int k = 0; k + 1 < no; k++) {
            const int la = lmk_index[kept[order[k]]], lb = lmk_index[kept[order[k + 1]]];
            o = out + cnt++;
            memset(o, 0, sizeof(*o));
            o->type = SADVIO_SPARSE_LMK_TO_LMK; o->kf = -1; o->lmk0 = la; o->lmk1 = lb;
            for (int a = 0; a < 3; a++) o->delta[a] = lp[3 * (size_t)la + a] - lp[3 * (size_t)lb + a];
            if (!nfr_sqrt_info(&S[specs[no + k].out_off], 3, false, o->sqrt_inf)) return fail();
        }
    }
    *n_out = cnt;
    return SADVIO_OK;
}

// sadvio_ba_get_prior: the handle's prior as it stands (J, r0: null = not asked for)
int read_prior(sadvio_ba_handle* h, sadvio_prior_info* info, double* J, double* r0) {
    const PriorState& PR = h->prior;
    if (info) { info->valid = PR.valid ? 1 : 0; info->n_full = PR.valid ? PR.n_full : 0; info->n = PR.valid ? PR.n : 0; info->form = PR.form; }
    if (!PR.valid) { if (J || r0) { h->err = "get_prior: the handle holds no prior"; return SADVIO_E_STATE; } return SADVIO_OK; }
    HIP_TRY(hipSetDevice(h->device));
    if (J) HIP_TRY(hipMemcpyAsync(J, PR.J.p, sizeof(double) * (size_t)PR.n_full * PR.n, hipMemcpyDeviceToHost, h->stream));
    if (r0) HIP_TRY(hipMemcpyAsync(r0, PR.r0.p, sizeof(double) * PR.n_full, hipMemcpyDeviceToHost, h->stream));
    HIP_TRY(hipStreamSynchronize(h->stream));
    return SADVIO_OK;
}

// sadvio_ba_set_prior: the caller's prior in place of the handle's (n_full <= 0: none)
int write_prior(sadvio_ba_handle* h, int32_t n_full, int32_t n, int32_t form, const double* J, const double* r0) {
    PriorState& PR = h->prior;
    PR.serial++;
    PR.hg_valid = false;
    if (n_full <= 0) { PR.valid = false; PR.z_valid = false; return SADVIO_OK; }
    if (n <= 0 || !J || !r0 || form != SADVIO_PRIOR_FORM_EIGEN) {   // a Cholesky-form prior carries its pivot order: only the device produces one
        h->err = "set_prior: needs J, r0 in the eigen form (orthogonal rows)"; return SADVIO_E_INVALID_ARG;
    }
    HIP_TRY(hipSetDevice(h->device));
    HIP_TRY(PR.J.alloc((size_t)n_full * n)); HIP_TRY(PR.r0.alloc(n_full));
    HIP_TRY(hipMemcpyAsync(PR.J.p, J, sizeof(double) * (size_t)n_full * n, hipMemcpyHostToDevice, h->stream));
    HIP_TRY(hipMemcpyAsync(PR.r0.p, r0, sizeof(double) * n_full, hipMemcpyHostToDevice, h->stream));
    HIP_TRY(hipStreamSynchronize(h->stream));
    PR.valid = true; PR.z_valid = false; PR.n_full = n_full; PR.n = n; PR.form = form; PR.cut_mode = SADVIO_EIG_CUT_REFERENCE;
    return SADVIO_OK;
}

}  // namespace
