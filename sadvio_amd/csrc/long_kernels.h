// long_kernels.h — long tracks: landmarks with more observations than a lane group of the tile kernels holds (MAX_LMK_OBS).
//
// The planner (layout_plan.h: layout_long) keeps such a landmark out of the tiles; inside every LM step it is linearised and
// eliminated by k_long_lin (beside k_build) and back-substituted by k_long_back (beside k_backsub), one workgroup of LONG_THREADS
// threads per track, thread t on observations t, t + LONG_THREADS, ... The arithmetic per observation and per landmark is the tile
// kernels' (lane_linearize, the damping of group_eliminate, the model cost change of k_backsub); what differs is where the sums
// are formed: H_ll and g_l over ALL observations first (registers, then a workgroup sum), then a second pass for what needs the
// inverse. Y[kf] = sum over the key-frame's observations of Jp^T Jl Li^T lives in LDS (18 doubles per observing key-frame); the
// Schur term -Y Y^T, the block diagonal, the gradients and the diagonal go to the window's accumulators with global FP64 atomics,
// like a global-mode tile's. A track of at most LONG_THREADS observations keeps its linearisation in registers between the passes;
// longer ones linearise twice. Not tuned: DESIGN.md "Long tracks".
//
// A long track that a prior keeps in the reduced system (lmk_const = 2; handles created with SADVIO_CFG_LONG_TRACK_PRIORS) stays on the
// long list: k_long_lin adds its pose-pose part and its cost and eliminates nothing, k_build_kept adds its rows and columns from the
// kept list, k_long_back takes its step from the reduced solution. DESIGN.md "Long tracks under a prior".
//
// Window totals: the linearisation's cost, fixed cost and gradient maximum are added to the k_build partial of the window's first
// tile (k_solve sums those; k_long_lin runs behind k_build on the stream), the back-substitution's four sums to the slot's IterAcc
// (behind k_solve, which zeroes them), as k_prior_m and k_line_eval do.
#pragma once
#include "kernels.h"

namespace sadvio {

// LDS of the two kernels: the Y strip (k_long_lin), the window's camera tables, the workgroup-sum exchange
constexpr int LONG_RED = 16;   // doubles a wave leaves for the workgroup sums
__host__ __device__ inline size_t long_lds_bytes(int n_kf) {
    return sizeof(double) * ((size_t)18 * n_kf + MAX_WIN_CAM * 17 + (LONG_THREADS / 64) * LONG_RED);
}

// The long list of the batch, a kernel argument of its own beside DevPtrs (which the tile kernels keep as they had it); part of the
// solve plan, so that n_long and the tables' addresses are in the key of the captured graph
struct LongArgs {
    int n_long, max_kf;   // tracks of the batch | most distinct key-frames observing one (LDS of k_long_lin)
    const int* rec;       // [n_long][LONG_REC] landmark | window | first entry of kf | key-frames | first entry of slot | observations
    const int* kf;        // distinct observing key-frames of every track (global indices, ascending)
    const int* slot;      // per observation of a track, in device order: index into the track's key-frame list
};

struct LongTrack {
    int gl, w, kf_off, n_kf, slot_off, n_obs;
};
__device__ __forceinline__ LongTrack long_track(const LongArgs& A, int i) {
    const int* r = A.rec + (long long)LONG_REC * i;
    return LongTrack{r[0], r[1], r[2], r[3], r[4], r[5]};
}

// Sum of n <= LONG_RED values per thread over the workgroup; every thread receives the totals (waves added in index order)
template <int N>
__device__ __forceinline__ void long_block_sum(double (&v)[N], double* red) {
    static_assert(N <= LONG_RED, "exchange area");
    const int wv = threadIdx.x >> 6, ln = threadIdx.x & 63;
    __syncthreads();   // the exchange area may still be read from the sum before
#pragma unroll
    for (int i = 0; i < N; i++) {
        const double s = wave_sum(v[i]);
        if (ln == 0) red[wv * LONG_RED + i] = s;
    }
    __syncthreads();
#pragma unroll
    for (int i = 0; i < N; i++) {
        double s = 0.0;
        for (int k = 0; k < LONG_THREADS / 64; k++) s += red[k * LONG_RED + i];
        v[i] = s;
    }
}

// Linearisation of observation o of a long track at the point of pose tables `ptab` (global, indexed by key-frame): lane_linearize
// with the key-frame itself as the slot and the free index as the row (-1: constant key-frame)
template <int FACTOR>
__device__ __forceinline__ void long_linearize(const DevPtrs& P, const double* ptab, const double* camTab, const WinDev& W, int o,
                                               const double* pw, bool keep_jl, bool lcounted, ObsLin& L) {
    ObsPre q = obs_prefetch<FACTOR>(P, o);
    q.slot = P.obs_kf[o];
    lane_linearize<FACTOR, true>(P, ptab, camTab, P.kf_fidx, W.cam_base, q, pw, keep_jl, lcounted, L);
    L.valid = true;
}

// ---- linearise and eliminate one long track per workgroup ------------------------------------------------------------------
template <int FACTOR>
__global__ __launch_bounds__(LONG_THREADS) void k_long_lin(DevPtrs P, LongArgs A, int slot) {
    extern __shared__ __attribute__((aligned(16))) char smem[];
    const LongTrack T = long_track(A, blockIdx.x);
    const LmState st = P.states[(long long)T.w * P.state_stride + slot];
    if (st.done) return;
    const WinDev W = P.win[T.w];
    const int tid = threadIdx.x;
    double* Y = (double*)smem;                       // [n_kf][6][3]
    double* camTab = Y + 18 * (size_t)A.max_kf;
    double* red = camTab + MAX_WIN_CAM * 17;
    stage_cams(P, W.cam_base, W.n_cam, camTab);
    for (int i = tid; i < 18 * T.n_kf; i += LONG_THREADS) Y[i] = 0.0;
    const int gl = T.gl, ob = P.lmk_ob[gl], oe = ob + T.n_obs;
    // 0 free (eliminated here), 1 constant, 2 kept in the reduced system by a prior (layout_reduced_plan: keep_landmark). A kept track
    // is not eliminated: as for a kept landmark of a tile (k_build), its pose-pose part goes the usual way with r~ = r, its observations
    // are counted in the cost, and its rows / columns, its gradient and its diagonal are added by k_build_kept, one thread per
    // observation. So it forms no H_ll, no g_l, no Y and no Schur pairs, writes no s_lmk and adds nothing to gmax here (the reduced
    // gradient carries g_l)
    const int lcode = P.lmk_const ? P.lmk_const[gl] : 0;
    const bool lfree = lcode == 0, lkept = lcode == 2;
    const double* xl = P.xl + (long long)st.cur * P.xl_stride + 3 * (long long)gl;
    const double pw[3] = {P.lmk_p[3 * (long long)gl] + xl[0], P.lmk_p[3 * (long long)gl + 1] + xl[1], P.lmk_p[3 * (long long)gl + 2] + xl[2]};
    const double* ptab = P.ptab + (long long)st.cur * P.ptab_stride;
    const bool single = T.n_obs <= LONG_THREADS;     // one observation per thread: its linearisation stays in registers
    __syncthreads();
    // pass 1: H_ll, g_l, the costs, over every observation
    double acc[11] = {0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0};   // H 6 | g 3 | cost | fixed cost
    ObsLin L;
    L.valid = false;
    for (int o = ob + tid; o < oe; o += LONG_THREADS) {
        long_linearize<FACTOR>(P, ptab, camTab, W, o, pw, lfree, lcode != 1, L);
        if (L.counted) acc[9] += L.rho;
        else { acc[10] += L.rho; L.r[0] = 0.0; L.r[1] = 0.0; }
        if (lkept) continue;   // the costs only
        acc[0] += L.Jl[0] * L.Jl[0] + L.Jl[3] * L.Jl[3];
        acc[1] += L.Jl[0] * L.Jl[1] + L.Jl[3] * L.Jl[4];
        acc[2] += L.Jl[0] * L.Jl[2] + L.Jl[3] * L.Jl[5];
        acc[3] += L.Jl[1] * L.Jl[1] + L.Jl[4] * L.Jl[4];
        acc[4] += L.Jl[1] * L.Jl[2] + L.Jl[4] * L.Jl[5];
        acc[5] += L.Jl[2] * L.Jl[2] + L.Jl[5] * L.Jl[5];
        acc[6] += L.Jl[0] * L.r[0] + L.Jl[3] * L.r[1];
        acc[7] += L.Jl[1] * L.r[0] + L.Jl[4] * L.r[1];
        acc[8] += L.Jl[2] * L.r[0] + L.Jl[5] * L.r[1];
    }
    long_block_sum(acc, red);
    const double* H = acc;
    const double* g = acc + 6;
    double Mi[6] = {0.0, 0.0, 0.0, 0.0, 0.0, 0.0}, gam[3];
    if (lfree) {
        double s[3];
        if (slot == 0) {
            s[0] = P.o.jacobi_scaling ? 1.0 / (1.0 + sqrt(H[0])) : 1.0;
            s[1] = P.o.jacobi_scaling ? 1.0 / (1.0 + sqrt(H[3])) : 1.0;
            s[2] = P.o.jacobi_scaling ? 1.0 / (1.0 + sqrt(H[5])) : 1.0;
            if (tid == 0) { P.s_lmk[3 * (long long)gl] = s[0]; P.s_lmk[3 * (long long)gl + 1] = s[1]; P.s_lmk[3 * (long long)gl + 2] = s[2]; }
        } else {
            s[0] = P.s_lmk[3 * (long long)gl]; s[1] = P.s_lmk[3 * (long long)gl + 1]; s[2] = P.s_lmk[3 * (long long)gl + 2];
        }
        damped_inverse(P, H, s, st.radius, Mi);
    }
    li_vec(Mi, g, gam);   // (zero unless the track is eliminated here)
    if (tid == 0) {
        // the window's totals: onto the k_build partial of its first tile (complete: k_build ran before this kernel)
        TileAcc* ta = P.tacc + (long long)(slot & 1) * P.n_tiles + W.tile_begin;
        atomic_add_f64(&ta->lin_cost, acc[9]);
        atomic_add_f64(&ta->fixed_cost, acc[10]);
        const double gm = lfree ? fmax(fabs(g[0]), fmax(fabs(g[1]), fabs(g[2]))) : 0.0;
        atomic_max_u64((unsigned long long*)&ta->gmax, (unsigned long long)__double_as_longlong(gm));   // non-negative doubles order like u64
    }
    // pass 2: what every observation on a free key-frame adds to the reduced system
    double* Sg = P.S + W.S_off;
    double* gredg = P.gred + W.red_off;
    double* gfullg = P.gfull + W.red_off;
    double* hdg = P.hdiag + W.red_off;
    const int dpf = W.dpf;
    for (int o = ob + tid; o < oe; o += LONG_THREADS) {
        if (!single) {
            long_linearize<FACTOR>(P, ptab, camTab, W, o, pw, lfree, lcode != 1, L);
            if (!L.counted) { L.r[0] = 0.0; L.r[1] = 0.0; }
        }
        if (L.row < 0) continue;   // constant key-frame
        // N = Jl Li^T and the reduced residual r~ = r - N gamma of an eliminated track; a constant or kept one has no elimination
        // term: gred = gfull
        double N[6] = {0.0, 0.0, 0.0, 0.0, 0.0, 0.0};
        double rt0 = L.r[0], rt1 = L.r[1];
        if (lfree) {
            li_row(Mi, L.Jl[0], L.Jl[1], L.Jl[2], N);
            li_row(Mi, L.Jl[3], L.Jl[4], L.Jl[5], N + 3);
            rt0 -= N[0] * gam[0] + N[1] * gam[1] + N[2] * gam[2];
            rt1 -= N[3] * gam[0] + N[4] * gam[1] + N[5] * gam[2];
        }
        const int base = L.row * dpf;
        double* y = Y + 18 * (size_t)A.slot[T.slot_off + (o - ob)];
#pragma unroll
        for (int i = 0; i < 6; i++) {
            const double j0 = L.Jp[i], j1 = L.Jp[6 + i];
            atomic_add_f64(&gredg[base + i], j0 * rt0 + j1 * rt1);
            atomic_add_f64(&gfullg[base + i], j0 * L.r[0] + j1 * L.r[1]);
            atomic_add_f64(&hdg[base + i], j0 * j0 + j1 * j1);
#pragma unroll
            for (int j = 0; j <= i; j++) atomic_add_f64(&Sg[s_index(W.ld, base + i, base + j)], j0 * L.Jp[j] + j1 * L.Jp[6 + j]);
            if (lfree) {
#pragma unroll
                for (int c = 0; c < 3; c++) atomic_add_f64(&y[3 * i + c], j0 * N[c] + j1 * N[3 + c]);
            }
        }
    }
    if (!lfree) return;   // a constant landmark couples nothing; a kept one couples through its own columns (k_build_kept)
    __syncthreads();
    // the Schur term -Y_a Y_b^T of every pair of free observing key-frames a >= b (the list ascends: so do their rows)
    const int wv = tid >> 6, ln = tid & 63;
    const int* kfl = A.kf + T.kf_off;
    for (int a = wv; a < T.n_kf; a += LONG_THREADS / 64) {
        const int fa = P.kf_fidx[kfl[a]];
        if (fa < 0) continue;
        for (int b = ln; b <= a; b += 64) {
            const int fb = P.kf_fidx[kfl[b]];
            if (fb < 0) continue;
            const double* ya = Y + 18 * (size_t)a;
            const double* yb = Y + 18 * (size_t)b;
            for (int i = 0; i < 6; i++)
                for (int j = 0; j < 6; j++) {
                    if (a == b && j > i) continue;
                    const double v = ya[3 * i] * yb[3 * j] + ya[3 * i + 1] * yb[3 * j + 1] + ya[3 * i + 2] * yb[3 * j + 2];
                    atomic_add_f64(&Sg[s_index(W.ld, fa * dpf + i, fb * dpf + j)], -v);
                }
        }
    }
}

// ---- back-substitution and candidate cost of one long track per workgroup ----------------------------------------------------
template <int FACTOR>
__global__ __launch_bounds__(LONG_THREADS) void k_long_back(DevPtrs P, LongArgs A, int slot) {
    extern __shared__ __attribute__((aligned(16))) char smem[];
    const LongTrack T = long_track(A, blockIdx.x);
    const long long so = (long long)T.w * P.state_stride + slot;
    const LmState st = P.states[so];
    // a step that was not taken (ended solve, failed factorisation) leaves no candidate and adds nothing, as k_backsub's tiles
    if (st.done || P.acc[so].chol_fail) return;
    const WinDev W = P.win[T.w];
    const int tid = threadIdx.x;
    double* camTab = (double*)smem;
    double* red = camTab + MAX_WIN_CAM * 17;
    stage_cams(P, W.cam_base, W.n_cam, camTab);
    const int gl = T.gl, ob = P.lmk_ob[gl], oe = ob + T.n_obs;
    // 0 free, 1 constant, 2 kept in the reduced system by a prior: its step is part of the reduced solution (k_solve counted |step|^2
    // there), so no H_ll, no t and no inverse are formed; |candidate|^2 is counted here, as k_backsub does for the kept landmarks of
    // its tiles (the long path runs on one device only: no rank to choose)
    const int lcode = P.lmk_const ? P.lmk_const[gl] : 0;
    const bool lfree = lcode == 0, lkept = lcode == 2;
    const int cur = st.cur;
    const double* xl = P.xl + (long long)cur * P.xl_stride + 3 * (long long)gl;
    double* xlc = P.xl + (long long)(1 - cur) * P.xl_stride + 3 * (long long)gl;
    const double p0[3] = {P.lmk_p[3 * (long long)gl], P.lmk_p[3 * (long long)gl + 1], P.lmk_p[3 * (long long)gl + 2]};
    const double x0[3] = {xl[0], xl[1], xl[2]};
    const double pw[3] = {p0[0] + x0[0], p0[1] + x0[1], p0[2] + x0[2]};
    const double* ptab = P.ptab + (long long)cur * P.ptab_stride;
    const double* ctab_all = P.ptab + (long long)(1 - cur) * P.ptab_stride;   // R | t at the candidate poses (k_solve's back half)
    const double* dp = P.delta + W.red_off;
    const bool single = T.n_obs <= LONG_THREADS;
    __syncthreads();
    // pass 1: H_ll and t = sum Jl^T (r + Jp dp)
    double acc[9] = {0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0};
    ObsLin L;
    L.valid = false;
    double e0 = 0.0, e1 = 0.0;   // predicted residual r + Jp dp of the observation
    // (a kept track needs none of the sums: the pass only leaves the linearisation in registers for pass 2, where it stays there)
    for (int o = ob + tid; o < oe && !(lkept && !single); o += LONG_THREADS) {
        long_linearize<FACTOR>(P, ptab, camTab, W, o, pw, lcode != 1, lcode != 1, L);
        if (!L.counted) { L.r[0] = 0.0; L.r[1] = 0.0; }
        e0 = L.r[0]; e1 = L.r[1];
        if (L.row >= 0) {
            const double* d = dp + L.row * W.dpf;
#pragma unroll
            for (int i = 0; i < 6; i++) { e0 += L.Jp[i] * d[i]; e1 += L.Jp[6 + i] * d[i]; }
        }
        if (lkept) continue;
        acc[0] += L.Jl[0] * L.Jl[0] + L.Jl[3] * L.Jl[3];
        acc[1] += L.Jl[0] * L.Jl[1] + L.Jl[3] * L.Jl[4];
        acc[2] += L.Jl[0] * L.Jl[2] + L.Jl[3] * L.Jl[5];
        acc[3] += L.Jl[1] * L.Jl[1] + L.Jl[4] * L.Jl[4];
        acc[4] += L.Jl[1] * L.Jl[2] + L.Jl[4] * L.Jl[5];
        acc[5] += L.Jl[2] * L.Jl[2] + L.Jl[5] * L.Jl[5];
        acc[6] += L.Jl[0] * e0 + L.Jl[3] * e1;
        acc[7] += L.Jl[1] * e0 + L.Jl[4] * e1;
        acc[8] += L.Jl[2] * e0 + L.Jl[5] * e1;
    }
    double d0, d1, d2;
    if (lkept) {   // (the same branch in every thread of the workgroup: no barrier of long_block_sum is skipped by some)
        // the landmark's step from the reduced solution (k_solve left it behind the poses' steps)
        const double* dr = dp + P.lmk_red[gl];
        d0 = dr[0]; d1 = dr[1]; d2 = dr[2];
    } else {
        long_block_sum(acc, red);
        double Mi[6] = {0.0, 0.0, 0.0, 0.0, 0.0, 0.0};
        if (lfree) {
            const double s[3] = {P.s_lmk[3 * (long long)gl], P.s_lmk[3 * (long long)gl + 1], P.s_lmk[3 * (long long)gl + 2]};
            damped_inverse(P, acc, s, st.radius, Mi);
        }
        // delta_l = -M^-1 t = -Li^T (Li t)
        double ut[3], vt[3];
        li_vec(Mi, acc + 6, ut);
        li_tvec(Mi, ut, vt);
        d0 = -vt[0]; d1 = -vt[1]; d2 = -vt[2];
    }
    const double c0 = x0[0] + d0, c1 = x0[1] + d1, c2 = x0[2] + d2;
    double sums[4] = {0.0, 0.0, 0.0, 0.0};   // candidate cost | model cost change | |step|^2 | |candidate|^2
    if (tid == 0) {
        xlc[0] = c0; xlc[1] = c1; xlc[2] = c2;
        if (lfree) { sums[2] = d0 * d0 + d1 * d1 + d2 * d2; sums[3] = c0 * c0 + c1 * c1 + c2 * c2; }
        else if (lkept) sums[3] = c0 * c0 + c1 * c1 + c2 * c2;
    }
    // pass 2: model cost change and the residual at the candidate of every block of the program
    const double pwc[3] = {p0[0] + c0, p0[1] + c1, p0[2] + c2};
    for (int o = ob + tid; o < oe; o += LONG_THREADS) {
        if (!single) {
            long_linearize<FACTOR>(P, ptab, camTab, W, o, pw, lcode != 1, lcode != 1, L);
            if (!L.counted) { L.r[0] = 0.0; L.r[1] = 0.0; }
            e0 = L.r[0]; e1 = L.r[1];
            if (L.row >= 0) {
                const double* d = dp + L.row * W.dpf;
#pragma unroll
                for (int i = 0; i < 6; i++) { e0 += L.Jp[i] * d[i]; e1 += L.Jp[6 + i] * d[i]; }
            }
        }
        if (!L.counted) continue;
        const double m0 = (e0 - L.r[0]) + L.Jl[0] * d0 + L.Jl[1] * d1 + L.Jl[2] * d2;
        const double m1 = (e1 - L.r[1]) + L.Jl[3] * d0 + L.Jl[4] * d1 + L.Jl[5] * d2;
        sums[1] += -m0 * (L.r[0] + 0.5 * m0) - m1 * (L.r[1] + 0.5 * m1);
        const int cam = P.obs_cam[o] - W.cam_base;
        const double* ct = camTab + cam * 17;
        const double* ctab = ctab_all + (long long)L.slot * POSE_TAB;
        double r[2];
        if (FACTOR == 0) {
            const double* m = P.obs_meas + 2 * (long long)o;
            pixel_factor<false>(ctab, ct, ct + 4, pwc, m[0], m[1], ct[16], r, nullptr, nullptr);
        } else {
            const double* m = P.obs_meas + 3 * (long long)o;
            double bb[3] = {m[0], m[1], m[2]};
            angular_factor<false>(ctab, ct + 4, pwc, bb, ct[16], r, nullptr, nullptr);
        }
        double sc_unused;
        sums[0] += huber_rho(P.o.huber_a, r[0] * r[0] + r[1] * r[1], sc_unused);
    }
    long_block_sum(sums, red);
    if (tid == 0) {
        IterAcc* a = P.acc + so;
        atomic_add_f64(&a->cand_cost, sums[0]);
        atomic_add_f64(&a->mcc, sums[1]);
        atomic_add_f64(&a->step_norm2, sums[2]);
        atomic_add_f64(&a->cand_norm2, sums[3]);
    }
}

}  // namespace sadvio
