// rel_kernels.h — sadvio_ba_marginalize_relative_batch, device side: the relative-pose information of MANY key-frame pairs of one
// window in one launch (what sadvio_ba_marginalize_relative computes pair by pair, marg_kernels.h: k_relmarg_*).
//
// One workgroup per pair (a, b). Its candidates are the distinct landmarks key-frame a observes, in window order (the handle's
// per-key-frame list, rel_driver.h); a candidate is an ITEM when key-frame b observes it too, with multiplicity = its features in b
// (marginalization.cpp:548-559). Amm is block diagonal, one 3 x 3 block per item:
//   phase 1   one thread per candidate: H_ll of the item (x multiplicity), its eigenvalues by cyclic Jacobi; the workgroup reduces the
//             largest |eigenvalue|, the item count and m = 3 * sum of multiplicities through LDS -> the cut on Amm
//   phase 2   REL_CH candidates at a time: wave 0 linearises them once more (one thread per candidate) and parks E (12 x 3), the
//             pseudo-inverse Pi (3 x 3) under the cut and the two 6 x 6 pose blocks in LDS; then 16 groups of 16 lanes, lane (i, j) owning the
//             3 x 3 block (i, j) of Ak, add H_pp - E Pi E^T of the rows r = group, group + 16, ... in that order
//   reduce    the 16 groups' partial Ak are summed in group order through LDS
//   tail      symmetrise from the lower triangle, 12 x 12 cyclic Jacobi, cut, Sigma_k, J of Relative6DPose(T_w_a, T_w_b, T_a_b, I),
//             J Sigma_k J^T and its Gauss-Jordan inverse — host_sym_eig / host_inverse of marg_driver.h restated on LDS arrays
// Every sum is taken in an order fixed by (the window, a, b) alone: no floating-point atomics, so a pair's bits depend neither on the
// other pairs of the batch nor on its position in it. Part of the library's single translation unit; not a public header.
#pragma once
#include "../../include/sadvio_ba.h"
#include "kernels.h"
#include "rel_runs.h"

namespace sadvio {

constexpr int REL_THREADS = 256;
constexpr int REL_CH = 64;                    // candidates per pass of phase 2 (one wave linearises them)
constexpr int REL_GROUPS = REL_THREADS / 16;  // 16 lanes per item: one 3 x 3 block of Ak each
constexpr int REL_ROW = 36 + 9 + 72;          // E | Pi | H_pp(a) H_pp(b); odd stride: thread-per-row stores hit distinct banks
// tail arrays inside the row buffer (doubles)
constexpr int REL_T_RED = 0, REL_T_AK = REL_GROUPS * 144, REL_T_A = REL_T_AK + 144, REL_T_V = REL_T_A + 144, REL_T_SK = REL_T_V + 144,
              REL_T_J = REL_T_SK + 144, REL_T_JS = REL_T_J + 72, REL_T_M = REL_T_JS + 72, REL_T_EV = REL_T_M + 72, REL_T_TAB = REL_T_EV + 12,
              REL_T_END = REL_T_TAB + 12;
static_assert(REL_T_END <= REL_CH * REL_ROW, "the tail's arrays live in the row buffer");
static_assert(3 * REL_THREADS + 48 <= REL_CH * REL_ROW, "phase 1 reduces through the row buffer");

struct RelDev {
    const int* kf_a; const int* kf_b;   // [n_pair] key-frame indices inside the window (checked on the host)
    int n_pair;
    int kf_base;                        // of the window
    int n_lmk_tot, n_obs_tot, n_cam_tot;   // bounds of everything the lists index
    const int* kf_ptr;                  // [n_kf + 1] per key-frame of the window: range in kf_lmk
    const int* kf_lmk;                  // distinct global landmarks the key-frame observes (pseudo-observations skipped), window order
    int n_kf_lmk;
    int noise_floor;                    // SADVIO_EIG_CUT_NOISE_FLOOR
    double* inf; double* Ak; double* Tab; int* n_shared; int* status;   // [n_pair][36 | 144 | 12 | 1 | 1]
};

// The reprojection factors of landmark gl in key-frames ga / gb at zero deltas (tabs: their pose tables). Returns the multiplicity (features
// in gb) when both observe it, else 0. Hll (registers) always; E (36) and Hp (72) are LDS rows, written when FULL. All x multiplicity.
template <int FACTOR, bool FULL>
__device__ __forceinline__ int rel_linearise(const DevPtrs& P, const RelDev& R, int gl, int ga, int gb, const double* tabs, double* Hll, double* E, double* Hp) {
#pragma unroll
    for (int i = 0; i < 9; i++) Hll[i] = 0.0;
    if (gl < 0 || gl >= R.n_lmk_tot) return 0;
    if (FULL) { for (int i = 0; i < 36; i++) E[i] = 0.0; for (int i = 0; i < 72; i++) Hp[i] = 0.0; }
    const double pw[3] = {P.lmk_p[3 * (long long)gl], P.lmk_p[3 * (long long)gl + 1], P.lmk_p[3 * (long long)gl + 2]};
    const int ob = max(P.lmk_ob[gl], 0), oe = min(P.lmk_oe[gl], R.n_obs_tot);
    int ca = 0, cb = 0;
    // a long track (handles created with SADVIO_CFG_LONG_TRACK_BATCH): the runs of ga and gb alone, by bisection (rel_runs.h) — the
    // observations the walk stops at, in its order. Every other landmark: one segment, the walk as it always was. (One copy of the
    // loop body: a second copy for the long tracks measured 2.3 % slower on windows without them, profiles/long_batch_time.txt.)
    int lo1 = oe, hi1 = oe, hi0 = oe;
    int o = ob;
    if (oe - ob > MAX_LMK_OBS) {
        const RelRuns rr = rel_runs(P.obs_kf, ob, oe, ga, gb);
        o = rr.lo[0]; hi0 = rr.hi[0]; lo1 = rr.lo[1]; hi1 = rr.hi[1];
    }
#pragma unroll 1
    for (int seg = 0; seg < 2; seg++, o = lo1, hi0 = hi1)
    for (; o < hi0; o++) {
        const int kf = P.obs_kf[o], cam = P.obs_cam[o];
        if (cam < 0 || cam >= R.n_cam_tot || (kf != ga && kf != gb)) continue;   // cam < 0: pseudo-observation of a sparse prior factor
        const int side = kf == ga ? 0 : 1;
        ca += side == 0; cb += side == 1;
        const double* tab = tabs + POSE_TAB * side;
        double r[2], Jp[12], Jl[6];
        if (FACTOR == 0) {
            const double* m = P.obs_meas + 2 * (long long)o;
            pixel_factor<true>(tab, P.cam_K + 4 * (long long)cam, P.cam_T + 12 * (long long)cam, pw, m[0], m[1], P.cam_isig[cam], r, Jp, Jl);
        } else {
            const double* m = P.obs_meas + 3 * (long long)o;
            const double bb[3] = {m[0], m[1], m[2]};
            angular_factor<true>(tab, P.cam_T + 12 * (long long)cam, pw, bb, P.cam_isig[cam], r, Jp, Jl);
        }
#pragma unroll
        for (int q = 0; q < 2; q++) {
#pragma unroll
            for (int a = 0; a < 3; a++) {
#pragma unroll
                for (int b = 0; b < 3; b++) Hll[3 * a + b] += Jl[3 * q + a] * Jl[3 * q + b];
                if (FULL) {
#pragma unroll
                    for (int p = 0; p < 6; p++) E[(6 * side + p) * 3 + a] += Jp[6 * q + p] * Jl[3 * q + a];
                }
            }
            if (FULL) {
#pragma unroll
                for (int p = 0; p < 6; p++)
#pragma unroll
                    for (int p2 = 0; p2 < 6; p2++) Hp[36 * side + 6 * p + p2] += Jp[6 * q + p] * Jp[6 * q + p2];
            }
        }
    }
    if (ca == 0 || cb == 0) return 0;
    const double mult = (double)cb;
#pragma unroll
    for (int i = 0; i < 9; i++) Hll[i] *= mult;
    if (FULL) { for (int i = 0; i < 36; i++) E[i] *= mult; for (int i = 0; i < 72; i++) Hp[i] *= mult; }
    return cb;
}

// cyclic Jacobi on the symmetrised 3 x 3 block (k_relmarg_lmk's loop): eigenvalues lam, eigenvectors in the columns of V
__device__ __forceinline__ void rel_jacobi3(const double* Hll, double* lam, double* V) {
    double A[9];
#pragma unroll
    for (int i = 0; i < 3; i++)
#pragma unroll
        for (int j = 0; j < 3; j++) { A[3 * i + j] = 0.5 * (Hll[3 * i + j] + Hll[3 * j + i]); V[3 * i + j] = i == j ? 1.0 : 0.0; }
    for (int sweep = 0; sweep < 30; sweep++) {
        const double off = A[1] * A[1] + A[2] * A[2] + A[5] * A[5], diag = A[0] * A[0] + A[4] * A[4] + A[8] * A[8];
        if (off <= 1e-60 || off <= 1e-32 * diag) break;
#pragma unroll
        for (int p = 0; p < 2; p++)
#pragma unroll
            for (int q = p + 1; q < 3; q++) {
                const double apq = A[3 * p + q];
                if (apq == 0.0) continue;
                const double theta = (A[3 * q + q] - A[3 * p + p]) / (2.0 * apq);
                const double t = (theta >= 0 ? 1.0 : -1.0) / (fabs(theta) + sqrt(theta * theta + 1.0));
                const double c = 1.0 / sqrt(t * t + 1.0), s = t * c;
#pragma unroll
                for (int k = 0; k < 3; k++) { const double a = A[3 * k + p], b = A[3 * k + q]; A[3 * k + p] = c * a - s * b; A[3 * k + q] = s * a + c * b; }
#pragma unroll
                for (int k = 0; k < 3; k++) { const double a = A[3 * p + k], b = A[3 * q + k]; A[3 * p + k] = c * a - s * b; A[3 * q + k] = s * a + c * b; }
#pragma unroll
                for (int k = 0; k < 3; k++) { const double a = V[3 * k + p], b = V[3 * k + q]; V[3 * k + p] = c * a - s * b; V[3 * k + q] = s * a + c * b; }
            }
    }
    lam[0] = A[0]; lam[1] = A[4]; lam[2] = A[8];
}

// host_sym_eig (marg_driver.h) for n = 12 on LDS arrays, one thread: A is overwritten, ev = its final diagonal, eigenvectors in V's columns
__device__ __forceinline__ void rel_jacobi12(double* A, double* V, double* ev) {
    const int n = 12;
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
                const double t = (theta >= 0 ? 1.0 : -1.0) / (fabs(theta) + sqrt(theta * theta + 1.0));
                const double c = 1.0 / sqrt(t * t + 1.0), s = t * c;
#pragma unroll
                for (int k = 0; k < n; k++) { const double a = A[k * n + p], b = A[k * n + q]; A[k * n + p] = c * a - s * b; A[k * n + q] = s * a + c * b; }
#pragma unroll
                for (int k = 0; k < n; k++) { const double a = A[p * n + k], b = A[q * n + k]; A[p * n + k] = c * a - s * b; A[q * n + k] = s * a + c * b; }
#pragma unroll
                for (int k = 0; k < n; k++) { const double a = V[k * n + p], b = V[k * n + q]; V[k * n + p] = c * a - s * b; V[k * n + q] = s * a + c * b; }
            }
    }
    for (int i = 0; i < n; i++) ev[i] = A[i * n + i];
}

// host_inverse (marg_driver.h) for n = 6 on the LDS array M = [A | I] (6 x 12), one thread; the inverse is left in M's right half.
// Fails on a pivot that is exactly zero (as the host routine) or not finite.
__device__ __forceinline__ bool rel_inverse6(double* M) {
    const int n = 6, w = 12;
    for (int c = 0; c < n; c++) {
        int p = c;
        for (int r = c + 1; r < n; r++) if (fabs(M[r * w + c]) > fabs(M[p * w + c])) p = r;
        const double piv = M[p * w + c];
        if (piv == 0.0 || !isfinite(piv)) return false;
        if (p != c) for (int j = 0; j < w; j++) { const double t = M[c * w + j]; M[c * w + j] = M[p * w + j]; M[p * w + j] = t; }
        const double d = 1.0 / M[c * w + c];
        for (int j = 0; j < w; j++) M[c * w + j] *= d;
        for (int r = 0; r < n; r++) {
            if (r == c) continue;
            const double f = M[r * w + c];
            if (f != 0.0) for (int j = 0; j < w; j++) M[r * w + j] -= f * M[c * w + j];
        }
    }
    return true;
}

// T_a_b = T_a_w T_w_b and J (6 x 12) of Relative6DPose(T_w_a, T_w_b, T_a_b, I) at zero deltas (k_relmarg_jac), one thread, into LDS.
// relative_pose_factor's Jacobian (device_math.h, residuals.hpp:70-131) for da = db = 0 and W = I, written block by block into the LDS
// array: its 6 x 15 local array, indexed in loops, would live in scratch memory.
__device__ __forceinline__ void rel_factor_jacobian(const double* Ta /*T_a_w*/, const double* Tb, double* Tab_out, double* J72) {
    double Twa[12], Twb[12], Tab[12], v[3];
#pragma unroll
    for (int i = 0; i < 3; i++)
#pragma unroll
        for (int j = 0; j < 3; j++) { Twa[3 * i + j] = Ta[3 * j + i]; Twb[3 * i + j] = Tb[3 * j + i]; }
    m3_tvec(Ta, Ta + 9, v);
#pragma unroll
    for (int i = 0; i < 3; i++) Twa[9 + i] = -v[i];
    m3_tvec(Tb, Tb + 9, v);
#pragma unroll
    for (int i = 0; i < 3; i++) Twb[9 + i] = -v[i];
    m3_mul(Ta, Twb, Tab);
    m3_vec(Ta, Twb + 9, v);
#pragma unroll
    for (int i = 0; i < 3; i++) Tab[9 + i] = v[i] + Ta[9 + i];
    // the factor's slots hold T_w_a, T_w_b (…Analytic.cpp:787-790): R = Rp^T Ra^T Rb, d = tb - ta
    const double z[3] = {0, 0, 0};
    double RaT_Rb[9], R[9], d[3], w[3];
    m3_tmul(Twa, Twb, RaT_Rb);
    m3_tmul(Tab, RaT_Rb, R);
#pragma unroll
    for (int i = 0; i < 3; i++) d[i] = Twb[9 + i] - Twa[9 + i];
    so3_log(R, w);
    double Jrw[9], Jrwi[9], Jr0[9], A[9], B[9], C[9], S[9], D1[9], D2[9], D3[9], D4[9], E2[9], F[9];
    so3_right_jacobian(w, Jrw); m3_inverse(Jrw, Jrwi);
    so3_right_jacobian(z, Jr0);
    m3_tmul(Twb, Twa, A); m3_mul(Jrwi, A, B); m3_mul(B, Jr0, C);
    so3_skew(d, S);
#pragma unroll
    for (int i = 0; i < 3; i++)
#pragma unroll
        for (int j = 0; j < 3; j++) D1[3 * i + j] = Tab[i] * Twa[3 * j] + Tab[3 + i] * Twa[3 * j + 1] + Tab[6 + i] * Twa[3 * j + 2];   // Rp^T Ra^T
    m3_mul(D1, S, D2); m3_mul(D2, Twa, D3); m3_mul(D3, Jr0, D4);
    m3_mul(Jrwi, Jr0, E2);
    m3_mul(D1, Twb, F);
#pragma unroll
    for (int i = 0; i < 3; i++)
#pragma unroll
        for (int j = 0; j < 3; j++) {
            J72[12 * i + j] = -C[3 * i + j];           J72[12 * i + 3 + j] = 0.0;
            J72[12 * i + 6 + j] = E2[3 * i + j];       J72[12 * i + 9 + j] = 0.0;
            J72[12 * (3 + i) + j] = D4[3 * i + j];     J72[12 * (3 + i) + 3 + j] = -Tab[3 * j + i];
            J72[12 * (3 + i) + 6 + j] = 0.0;           J72[12 * (3 + i) + 9 + j] = F[3 * i + j];
        }
#pragma unroll
    for (int i = 0; i < 12; i++) Tab_out[i] = Tab[i];
}

template <int FACTOR>
__global__ __launch_bounds__(REL_THREADS) void k_rel_batch(DevPtrs P, RelDev R) {
    __shared__ double rows[REL_CH * REL_ROW];
    __shared__ double s_tab[2 * POSE_TAB];
    __shared__ int s_item[REL_CH];
    __shared__ double s_cut;
    __shared__ int s_nitems, s_ok;
    const int pair = blockIdx.x, tid = threadIdx.x;
    if (pair >= R.n_pair) return;
    const int a = R.kf_a[pair], b = R.kf_b[pair];
    const int ga = R.kf_base + a, gb = R.kf_base + b;
    const int c_begin = max(R.kf_ptr[a], 0), c_end = min(R.kf_ptr[a + 1], R.n_kf_lmk);
    const int n_cand = max(c_end - c_begin, 0);
    if (tid < 2) {
        const double d6[6] = {0, 0, 0, 0, 0, 0};
        double tab[POSE_TAB];
        pose_table_entry(P.kf_T0 + 12 * (long long)(tid == 0 ? ga : gb), d6, tab);
#pragma unroll
        for (int i = 0; i < POSE_TAB; i++) s_tab[POSE_TAB * tid + i] = tab[i];
    }
    __syncthreads();

    // ---- phase 1: largest |eigenvalue| of all blocks, item count, m ----
    {
        double lmax = 0.0;
        int n_it = 0, mm = 0;
        for (int c = tid; c < n_cand; c += REL_THREADS) {
            double Hll[9], lam[3], V[9];
            const int cb = rel_linearise<FACTOR, false>(P, R, R.kf_lmk[c_begin + c], ga, gb, s_tab, Hll, nullptr, nullptr);
            if (cb == 0) continue;
            rel_jacobi3(Hll, lam, V);
            lmax = fmax(lmax, fmax(fabs(lam[0]), fmax(fabs(lam[1]), fabs(lam[2]))));
            n_it += 1; mm += 3 * cb;
        }
        rows[tid] = lmax; rows[REL_THREADS + tid] = (double)n_it; rows[2 * REL_THREADS + tid] = (double)mm;   // (counts: exact in a double)
        __syncthreads();
        double* part = rows + 3 * REL_THREADS;   // [3][16]
        if (tid < 16) {
            double mx = 0.0, ni = 0.0, ms = 0.0;
            for (int k = 0; k < 16; k++) { mx = fmax(mx, rows[16 * tid + k]); ni += rows[REL_THREADS + 16 * tid + k]; ms += rows[2 * REL_THREADS + 16 * tid + k]; }
            part[tid] = mx; part[16 + tid] = ni; part[32 + tid] = ms;
        }
        __syncthreads();
        if (tid == 0) {
            double mx = 0.0, ni = 0.0, ms = 0.0;
            for (int k = 0; k < 16; k++) { mx = fmax(mx, part[k]); ni += part[16 + k]; ms += part[32 + k]; }
            s_nitems = (int)ni;
            s_cut = R.noise_floor ? fmax(1e-12, ms * 2.220446049250313e-16 * mx) : 1e-12;   // SADVIO_EIG_CUT_* on Amm (k_relmarg_apply)
        }
        __syncthreads();
    }
    const int n_items = s_nitems;
    const double cut_mm = s_cut;
    double* const oinf = R.inf + 36 * (long long)pair;
    double* const oAk = R.Ak + 144 * (long long)pair;
    double* const oTab = R.Tab + 12 * (long long)pair;
    if (n_items == 0) {   // the two key-frames share no landmark: refused, zeros (uniform over the workgroup)
        if (tid < 144) oAk[tid] = 0.0;
        if (tid < 36) oinf[tid] = 0.0;
        if (tid < 12) oTab[tid] = 0.0;
        if (tid == 0) { R.n_shared[pair] = 0; R.status[pair] = SADVIO_E_REFUSED; }
        return;
    }

    // ---- phase 2: Ak = sum over the items of H_pp - E Pi E^T, lane (bi, bj) of a group owns the 3 x 3 block (bi, bj) ----
    const int grp = tid >> 4, bi = (tid >> 2) & 3, bj = tid & 3;
    double acc[9];
#pragma unroll
    for (int i = 0; i < 9; i++) acc[i] = 0.0;
    for (int c0 = 0; c0 < n_cand; c0 += REL_CH) {
        if (tid < REL_CH) {
            int item = 0;
            const int c = c0 + tid;
            if (c < n_cand) {
                double* row = rows + REL_ROW * tid;
                double Hll[9], lam[3], V[9];
                const int cb = rel_linearise<FACTOR, true>(P, R, R.kf_lmk[c_begin + c], ga, gb, s_tab, Hll, row, row + 45);
                if (cb > 0) {
                    item = 1;
                    rel_jacobi3(Hll, lam, V);
                    double Pi[9] = {0, 0, 0, 0, 0, 0, 0, 0, 0};
#pragma unroll
                    for (int k = 0; k < 3; k++) {
                        if (!(lam[k] > cut_mm)) continue;
                        const double iv = 1.0 / lam[k];
#pragma unroll
                        for (int i = 0; i < 3; i++)
#pragma unroll
                            for (int j = 0; j < 3; j++) Pi[3 * i + j] += V[3 * i + k] * iv * V[3 * j + k];
                    }
#pragma unroll
                    for (int i = 0; i < 9; i++) row[36 + i] = Pi[i];
                }
            }
            s_item[tid] = item;
        }
        __syncthreads();
        for (int r = grp; r < REL_CH; r += REL_GROUPS) {
            if (!s_item[r]) continue;
            const double* row = rows + REL_ROW * r;
            const double* Ei = row + 9 * bi;    // rows 3 bi .. 3 bi + 2 of E (12 x 3)
            const double* Ej = row + 9 * bj;
            const double* Pi = row + 36;
            const bool same = (bi >> 1) == (bj >> 1);
            const double* Hp = row + 45 + 36 * (bi >> 1) + 18 * (bi & 1) + 3 * (bj & 1);   // block (bi, bj) of this side's 6 x 6
#pragma unroll
            for (int i = 0; i < 3; i++) {
                double t[3];
#pragma unroll
                for (int k = 0; k < 3; k++) t[k] = Ei[3 * i] * Pi[k] + Ei[3 * i + 1] * Pi[3 + k] + Ei[3 * i + 2] * Pi[6 + k];
#pragma unroll
                for (int j = 0; j < 3; j++) {
                    const double s = t[0] * Ej[3 * j] + t[1] * Ej[3 * j + 1] + t[2] * Ej[3 * j + 2];
                    acc[3 * i + j] += (same ? Hp[6 * i + j] : 0.0) - s;
                }
            }
        }
        __syncthreads();
    }

    // ---- the 16 groups' partial sums, in group order ----
    double* const t_red = rows + REL_T_RED; double* const t_Ak = rows + REL_T_AK; double* const t_A = rows + REL_T_A; double* const t_V = rows + REL_T_V;
    double* const t_Sk = rows + REL_T_SK; double* const t_J = rows + REL_T_J; double* const t_JS = rows + REL_T_JS; double* const t_M = rows + REL_T_M;
    double* const t_ev = rows + REL_T_EV; double* const t_Tab = rows + REL_T_TAB;
#pragma unroll
    for (int i = 0; i < 3; i++)
#pragma unroll
        for (int j = 0; j < 3; j++) t_red[144 * grp + 12 * (3 * bi + i) + 3 * bj + j] = acc[3 * i + j];
    __syncthreads();
    if (tid < 144) {
        double s = 0.0;
        for (int g = 0; g < REL_GROUPS; g++) s += t_red[144 * g + tid];
        t_Ak[tid] = s;
    }
    __syncthreads();

    // ---- tail: rankReveallingDecomposition (Eigen reads the lower triangle) -> Sigma_k -> inf = (J Sigma_k J^T)^-1 ----
    if (tid < 144) { const int i = tid / 12, j = tid - 12 * i; t_A[tid] = j <= i ? t_Ak[tid] : t_Ak[12 * j + i]; }
    if (tid == 64) rel_factor_jacobian(P.kf_T0 + 12 * (long long)ga, P.kf_T0 + 12 * (long long)gb, t_Tab, t_J);   // (wave 1, beside the Jacobi of wave 0)
    __syncthreads();
    if (tid == 0) {
        rel_jacobi12(t_A, t_V, t_ev);
        double mx = 0.0;
        for (int k = 0; k < 12; k++) mx = fmax(mx, fabs(t_ev[k]));
        s_cut = R.noise_floor ? fmax(1e-12, 12 * 2.220446049250313e-16 * mx * (2.0 + n_items)) : 1e-12;   // SADVIO_EIG_CUT_* on Ak
    }
    __syncthreads();
    const double cut_k = s_cut;
    if (tid < 144) {
        const int i = tid / 12, j = tid - 12 * i;
        double s = 0.0;
        for (int k = 0; k < 12; k++) {
            if (!(t_ev[k] > cut_k)) continue;
            const double iv = 1.0 / t_ev[k];
            s += t_V[12 * i + k] * iv * t_V[12 * j + k];
        }
        t_Sk[tid] = s;
    }
    __syncthreads();
    if (tid < 72) {
        const int i = tid / 12, j = tid - 12 * i;
        double s = 0.0;
        for (int k = 0; k < 12; k++) s += t_J[12 * i + k] * t_Sk[12 * k + j];
        t_JS[tid] = s;
    }
    __syncthreads();
    if (tid < 72) {   // M = [J Sigma_k J^T | I]
        const int i = tid / 12, j = tid - 12 * i;
        double s = 0.0;
        if (j < 6) { for (int k = 0; k < 12; k++) s += t_JS[12 * i + k] * t_J[12 * j + k]; }
        else s = (j - 6) == i ? 1.0 : 0.0;
        t_M[tid] = s;
    }
    __syncthreads();
    if (tid == 0) s_ok = rel_inverse6(t_M) ? 1 : 0;
    __syncthreads();
    const bool ok = s_ok != 0;   // a failed inverse: refused, zeros
    if (tid < 144) oAk[tid] = ok ? t_Ak[tid] : 0.0;
    if (tid < 36) { const int i = tid / 6, j = tid - 6 * i; oinf[tid] = ok ? t_M[12 * i + 6 + j] : 0.0; }
    if (tid < 12) oTab[tid] = ok ? t_Tab[tid] : 0.0;
    if (tid == 0) { R.n_shared[pair] = ok ? n_items : 0; R.status[pair] = ok ? SADVIO_OK : SADVIO_E_REFUSED; }
}

}  // namespace sadvio
