// cov_long_kernels.h — sadvio_ba_covariance on windows with long tracks (handles created with SADVIO_CFG_LONG_TRACK_COVARIANCE).
//
// The planner keeps a long track out of the landmark tiles (long_kernels.h), so k_cov_assemble / k_cov_assemble_sqrt never see it.
// Two kernels here do for it what those and k_cov_lmk do for a landmark of the tiles, one workgroup of LONG_THREADS per track over
// the window's slice of the long list (HostWin::long_begin / long_end):
//   k_cov_long<FACTOR, SQRT>   behind the tile assembly, in front of k_cov_schur(_sqrt): fills the track's rows of the tables of
//                              CovDev (and CovSqrtDev) at its own observation range, exactly the layout the tile assembly leaves, so
//                              that k_cov_schur, k_cov_schur_sqrt, k_cov_kept, k_cov_cross and k_cov_innov read a long track like any
//                              landmark. Entries are the free observing key-frames in device observation order (a long track's
//                              observations are sorted by key-frame: LongArgs::kf / slot).
//   k_cov_lmk_long<SQRT>       behind the inversion: the track's landmark block. k_cov_lmk skips the landmarks k_cov_long marked
//                              (CovDev::is_long) — its n^2 ordered pairs on 64 lanes would be 4 096 dependent passes at n = 512.
// Where the sums are formed (no floating-point atomic, every order fixed: two calls give the same bits):
//   over all observations (H_ll; |column|^2 and the Gram-Schmidt dot products of the square-root form): thread t takes observations
//     t, t + LONG_THREADS, .., then long_block_sum — a butterfly inside each wave, the waves added in index order;
//   per observing key-frame (H_lp, sum Jp^T Jp; C_a): ONE owner thread per entry walks that key-frame's run of observations in order;
//   over the entries of the landmark block: thread e forms T_e = sum_f Sigma_pp(c_e, c_f) W_f^T with f ascending and W_e T_e, thread
//     t adds its entries t, t + LONG_THREADS, .., then long_block_sum.
// Every observation is linearised at x* by cov_obs_jacobians, as the tile assembly does it (same Huber corrector, same treatment of
// a failed projection). Nothing per observation lives in registers beyond the one in hand: the plain form linearises a second time in
// the owner pass, the square-root form keeps J_p and Q1 in CovSqrtDev::jp / q (global memory, each row written and rewritten by the
// thread that owns its observation). Not tuned: a key-frame that holds very many of a track's observations serialises on its owner.
// Both kernels are wrappers of a __device__ body (cov_long_body, cov_lmk_long_body) that takes the track; the unit kernels of
// sadvio_ba_covariance_batch (cov_batch_kernels.h: k_covb_long, k_covb_lmk_long) call the plain forms of the same bodies.
// Part of the library's single translation unit; not a public header.
#pragma once
#include "cov_kernels.h"
#include "long_kernels.h"

namespace sadvio {

// LDS of k_cov_long: the workgroup-sum exchange | entry of every observing key-frame (-1: constant) | first observation of every
// key-frame's run (+ one past the last) | the entry count
__host__ __device__ inline size_t cov_long_lds_bytes(int n_kf) {
    return sizeof(double) * (LONG_THREADS / 64) * LONG_RED + sizeof(int) * (2 * (size_t)n_kf + 2);
}
static_assert(sizeof(double) * (LONG_THREADS / 64) * LONG_RED + sizeof(int) * (2 * (size_t)MAX_LONG_KF + 2) <= 64 * 1024,
              "k_cov_long is launched without raising the dynamic LDS limit");

// The body of k_cov_long for track T of the long list, by its workgroup of LONG_THREADS; smem: cov_long_lds_bytes(A.max_kf) of LDS.
// k_covb_long (cov_batch_kernels.h) calls the plain form with its unit's CovDev: one body, so a track's bits are the single call's.
template <int FACTOR, bool SQRT>
__device__ __forceinline__ void cov_long_body(const DevPtrs& P, const CovDev& C, const CovSqrtDev& Q1, const LongArgs& A, const LongTrack& T, char* smem) {
    const WinDev W = P.win[C.w];
    const int tid = threadIdx.x;
    double* red = (double*)smem;
    int* ent_of = (int*)(red + (LONG_THREADS / 64) * LONG_RED);   // [max_kf]
    int* run = ent_of + A.max_kf;                                 // [max_kf + 1], then the entry count
    const int gl = T.gl, l = gl - W.lmk_base, ob = P.lmk_ob[gl], m = T.n_obs;
    const long long e0 = ob - W.obs_base;
    const int* slot = A.slot + T.slot_off;
    const int* kfl = A.kf + T.kf_off;
    for (int s = tid; s < T.n_kf; s += LONG_THREADS) ent_of[s] = P.kf_fidx[kfl[s]] >= 0 ? 1 : 0;
    for (int i = tid; i < m; i += LONG_THREADS)
        if (i == 0 || slot[i] != slot[i - 1]) run[slot[i]] = i;
    __syncthreads();
    if (tid == 0) {   // entries in first-appearance order of the free key-frames
        int n = 0;
        for (int s = 0; s < T.n_kf; s++) ent_of[s] = ent_of[s] ? n++ : -1;
        run[T.n_kf] = m;
        run[A.max_kf + 1] = n;
    }
    __syncthreads();
    const int n_ent = run[A.max_kf + 1];
    const double* xl = P.xl + (long long)C.cur * P.xl_stride + 3 * (long long)gl;
    const double pw[3] = {P.lmk_p[3 * (long long)gl] + xl[0], P.lmk_p[3 * (long long)gl + 1] + xl[1], P.lmk_p[3 * (long long)gl + 2] + xl[2]};
    const int lc = P.lmk_const ? P.lmk_const[gl] : 0;   // 0 free | 1 constant | 2 kept in the reduced system
    int status = lc == 1 ? COV_LMK_CONST : (lc == 2 ? COV_LMK_REDUCED : COV_LMK_ELIMINATED);
    if constexpr (!SQRT) {
        double H[6] = {0.0, 0.0, 0.0, 0.0, 0.0, 0.0};
        for (int i = tid; i < m; i += LONG_THREADS) {
            double Jp[12], Jl[6];
            cov_obs_jacobians<FACTOR>(P, C, ob + i, pw, Jp, Jl);
            H[0] += Jl[0] * Jl[0] + Jl[3] * Jl[3]; H[1] += Jl[0] * Jl[1] + Jl[3] * Jl[4]; H[2] += Jl[0] * Jl[2] + Jl[3] * Jl[5];
            H[3] += Jl[1] * Jl[1] + Jl[4] * Jl[4]; H[4] += Jl[1] * Jl[2] + Jl[4] * Jl[5]; H[5] += Jl[2] * Jl[2] + Jl[5] * Jl[5];
        }
        long_block_sum(H, red);   // every thread holds the same H from here on: what follows branches uniformly
        double Hi[6] = {0.0, 0.0, 0.0, 0.0, 0.0, 0.0};
        if (status == COV_LMK_ELIMINATED && !(m >= 2 && cov_sym3_inverse(H, Hi))) status = COV_LMK_SINGULAR;
        for (int s = tid; s < T.n_kf; s += LONG_THREADS) {   // one owner per entry, over its key-frame's observations in order
            const int e = ent_of[s];
            if (e < 0) continue;
            double w18[COV_ENT_W], h21[COV_ENT_HPP];
#pragma unroll
            for (int q = 0; q < COV_ENT_W; q++) w18[q] = 0.0;
#pragma unroll
            for (int q = 0; q < COV_ENT_HPP; q++) h21[q] = 0.0;
            for (int i = run[s]; i < run[s + 1]; i++) {
                double Jp[12], Jl[6];
                cov_obs_jacobians<FACTOR>(P, C, ob + i, pw, Jp, Jl);
#pragma unroll
                for (int a = 0; a < 3; a++)
#pragma unroll
                    for (int c = 0; c < 6; c++) w18[6 * a + c] += Jl[a] * Jp[c] + Jl[3 + a] * Jp[6 + c];
#pragma unroll
                for (int a = 0; a < 6; a++)
#pragma unroll
                    for (int c = 0; c <= a; c++) h21[a * (a + 1) / 2 + c] += Jp[a] * Jp[c] + Jp[6 + a] * Jp[6 + c];
            }
            double* wo = C.ent_w + (e0 + e) * COV_ENT_W;
            double* ho = C.ent_hpp + (e0 + e) * COV_ENT_HPP;
#pragma unroll
            for (int c = 0; c < 6; c++) {   // H_lp -> W = H_ll^-1 H_lp (zero for a track that is not eliminated)
                double y[3] = {0.0, 0.0, 0.0};
                if (status == COV_LMK_ELIMINATED) cov_sym3_vec(Hi, w18[c], w18[6 + c], w18[12 + c], y);
                wo[c] = y[0]; wo[6 + c] = y[1]; wo[12 + c] = y[2];
            }
#pragma unroll
            for (int q = 0; q < COV_ENT_HPP; q++) ho[q] = h21[q];
            C.ent_col[e0 + e] = P.kf_fidx[kfl[s]] * W.dpf;
        }
        if (tid == 0)
            for (int q = 0; q < 6; q++) { C.hll[6 * (long long)l + q] = H[q]; C.hinv[6 * (long long)l + q] = Hi[q]; }
    } else {
        const bool elim = status == COV_LMK_ELIMINATED;
        double* Q = Q1.q + 6 * e0;         // row r of the track at Q[3 r]: rows 2 i, 2 i + 1 are observation i's, thread i % LONG_THREADS's
        double* JP = Q1.jp + 12 * e0;
        int* EN = Q1.ent + e0;
        double cn[3] = {0.0, 0.0, 0.0};    // |column|^2 of J_l
        for (int i = tid; i < m; i += LONG_THREADS) {
            double Jp[12], Jl[6];
            cov_obs_jacobians<FACTOR>(P, C, ob + i, pw, Jp, Jl);
            for (int q = 0; q < 12; q++) JP[12 * i + q] = Jp[q];
            for (int q = 0; q < 6; q++) Q[6 * i + q] = elim ? Jl[q] : 0.0;
            for (int c = 0; c < 3; c++) cn[c] += Jl[c] * Jl[c] + Jl[3 + c] * Jl[3 + c];
            EN[i] = ent_of[slot[i]];
        }
        long_block_sum(cn, red);
        double R[6] = {0.0, 0.0, 0.0, 0.0, 0.0, 0.0};
        if (elim) {   // Gram-Schmidt of k_cov_assemble_sqrt, its column sums over 2 m rows as workgroup sums (uniform branches throughout)
            const double tol = 64.0 * 2.220446049250313e-16;
            bool ok = m >= 2;
            for (int j = 0; j < 3 && ok; j++) {
                for (int pass = 0; pass < 2; pass++)
                    for (int k = 0; k < j; k++) {
                        double s[1] = {0.0};
                        for (int i = tid; i < m; i += LONG_THREADS) s[0] += Q[6 * i + k] * Q[6 * i + j] + Q[6 * i + 3 + k] * Q[6 * i + 3 + j];
                        long_block_sum(s, red);
                        for (int i = tid; i < m; i += LONG_THREADS) { Q[6 * i + j] -= s[0] * Q[6 * i + k]; Q[6 * i + 3 + j] -= s[0] * Q[6 * i + 3 + k]; }
                        R[k == 0 ? j : 3 + j - 1] += s[0];   // (0, j) | (1, 2)
                    }
                double nn[1] = {0.0};
                for (int i = tid; i < m; i += LONG_THREADS) nn[0] += Q[6 * i + j] * Q[6 * i + j] + Q[6 * i + 3 + j] * Q[6 * i + 3 + j];
                long_block_sum(nn, red);
                if (!(nn[0] > tol * cn[j])) { ok = false; break; }
                const double rjj = sqrt(nn[0]);
                R[j == 0 ? 0 : (j == 1 ? 3 : 5)] = rjj;
                for (int i = tid; i < m; i += LONG_THREADS) { Q[6 * i + j] /= rjj; Q[6 * i + 3 + j] /= rjj; }
            }
            if (!ok) status = COV_LMK_SINGULAR;
        }
        __syncthreads();   // the owners read rows other threads wrote
        for (int s = tid; s < T.n_kf; s += LONG_THREADS) {   // C_a = Q1^T J_p,a, observation after observation
            const int e = ent_of[s];
            if (e < 0) continue;
            double c18[COV_ENT_W];
#pragma unroll
            for (int q = 0; q < COV_ENT_W; q++) c18[q] = 0.0;
            if (status == COV_LMK_ELIMINATED)
                for (int i = run[s]; i < run[s + 1]; i++) {
                    const double* q = Q + 6 * i;
                    const double* jp = JP + 12 * i;
#pragma unroll
                    for (int a = 0; a < 3; a++)
#pragma unroll
                        for (int c = 0; c < 6; c++) c18[6 * a + c] += q[a] * jp[c] + q[3 + a] * jp[6 + c];
                }
            double* co = C.ent_w + (e0 + e) * COV_ENT_W;
#pragma unroll
            for (int q = 0; q < COV_ENT_W; q++) co[q] = c18[q];
            C.ent_col[e0 + e] = P.kf_fidx[kfl[s]] * W.dpf;
        }
        if (tid == 0)
            for (int q = 0; q < 6; q++) C.hll[6 * (long long)l + q] = R[q];
    }
    if (tid == 0) {
        C.status[l] = status;
        C.ent_n[l] = status == COV_LMK_SINGULAR ? 0 : n_ent;
        C.is_long[l] = 1;
    }
}

template <int FACTOR, bool SQRT>
__global__ __launch_bounds__(LONG_THREADS) void k_cov_long(DevPtrs P, CovDev C, CovSqrtDev Q1, LongArgs A, int first) {
    extern __shared__ __attribute__((aligned(16))) char smem[];
    cov_long_body<FACTOR, SQRT>(P, C, Q1, A, long_track(A, first + blockIdx.x), smem);
}

// The body of k_cov_lmk_long for track T; red: the workgroup-sum exchange in LDS. k_covb_lmk_long calls the plain form.
template <bool SQRT>
__device__ __forceinline__ void cov_lmk_long_body(const DevPtrs& P, const CovDev& C, const LongTrack& T, double* red) {
    const WinDev W = P.win[C.w];
    const int l = T.gl - W.lmk_base;
    const int status = C.status[l];
    const int n = status == COV_LMK_ELIMINATED ? C.ent_n[l] : 0;
    const long long e0 = P.lmk_ob[T.gl] - W.obs_base;
    double acc[9];
#pragma unroll
    for (int i = 0; i < 9; i++) acc[i] = 0.0;
    for (int e = threadIdx.x; e < n; e += LONG_THREADS) {
        const double* Se = C.Sig + (long long)C.ent_col[e0 + e] * C.Np;
        double Te[18];   // T_e (6 x 3) = sum_f Sigma_pp(c_e, c_f) W_f^T, f ascending
#pragma unroll
        for (int i = 0; i < 18; i++) Te[i] = 0.0;
        for (int f = 0; f < n; f++) {
            const double* Sg = Se + C.ent_col[e0 + f];
            const double* Wf = C.ent_w + (e0 + f) * COV_ENT_W;
            double wf[18];
#pragma unroll
            for (int i = 0; i < 18; i++) wf[i] = Wf[i];
#pragma unroll
            for (int k = 0; k < 6; k++) {
                double s[6];
#pragma unroll
                for (int g = 0; g < 6; g++) s[g] = Sg[(long long)k * C.Np + g];
#pragma unroll
                for (int j = 0; j < 3; j++) {
                    double v = 0.0;
#pragma unroll
                    for (int g = 0; g < 6; g++) v += s[g] * wf[6 * j + g];
                    Te[3 * k + j] += v;
                }
            }
        }
        const double* We = C.ent_w + (e0 + e) * COV_ENT_W;
#pragma unroll
        for (int i = 0; i < 3; i++)
#pragma unroll
            for (int j = 0; j < 3; j++) {
                double v = 0.0;
#pragma unroll
                for (int k = 0; k < 6; k++) v += We[6 * i + k] * Te[3 * k + j];
                acc[3 * i + j] += v;
            }
    }
    long_block_sum(acc, red);
    if (threadIdx.x == 0) cov_lmk_write<SQRT>(P, C, W, l, status, acc);
}

template <bool SQRT>
__global__ __launch_bounds__(LONG_THREADS) void k_cov_lmk_long(DevPtrs P, CovDev C, LongArgs A, int first) {
    __shared__ double red[(LONG_THREADS / 64) * LONG_RED];
    cov_lmk_long_body<SQRT>(P, C, long_track(A, first + blockIdx.x), red);
}

}  // namespace sadvio
