// solve_driver.h — the launch sequence of sadvio_ba_solve, in two halves:
//   plan_solve     decides everything a solve launches with (geometry, LDS bytes, kernel variants, routes of the out-of-LDS windows,
//                  workspace pointers), allocates what it needs and may synchronise the stream; nothing is launched from it
//   enqueue_solve  launches, reading only the plan: it may run under stream capture, so it neither allocates nor synchronises
// The bytes of the plan are the key of the captured graph: what enqueue_solve reads and what decides a re-capture are one thing.
// Beside them the other steps of sadvio_ba_solve (convert_options, launch_solve with the graph capture, solve_summaries) and the
// read-backs of a solved batch (read_deltas, read_line_deltas, read_trace).
// Part of the library's single translation unit (ba_capi.hip); not a public header.
#pragma once
#include <cstddef>
#include <type_traits>

#include "ba_handle.h"
#include "solve_opts.h"

namespace {

DevPtrs make_ptrs(sadvio_ba_handle* h, const SolveOpts& o, int state_stride) {
    DevPtrs P{};
    P.win = h->d_win.p; P.tiles = h->d_tiles.p;
    P.kf_T0 = h->d_kf_T0.p; P.kf_fidx = h->d_kf_fidx.p;
    P.xp = h->d_xp.p; P.xv = h->d_xv.p; P.xba = h->d_xba.p; P.xbg = h->d_xbg.p;
    P.xp_stride = 6LL * h->plan.n_kf_tot; P.xv_stride = 3LL * h->plan.n_kf_tot; P.xl_stride = 3LL * h->plan.n_lmk_tot;
    P.kf_vel = h->d_kf_vel.p; P.kf_ba = h->d_kf_ba.p; P.kf_bg = h->d_kf_bg.p;
    P.cam_K = h->d_cam_K.p; P.cam_T = h->d_cam_T.p; P.cam_isig = h->d_cam_isig.p;
    P.lmk_p = h->d_lmk_p.p; P.xl = h->d_xl.p; P.s_lmk = h->d_s_lmk.p;
    P.lmk_const = h->plan.has_lmk_const ? h->d_lmk_const.p : nullptr;
    P.lmk_ob = h->d_lmk_ob.p; P.lmk_oe = h->d_lmk_oe.p;
    P.obs_kf = h->d_obs_kf.p; P.obs_cam = h->d_obs_cam.p; P.obs_meas = h->d_obs_meas.p;
    P.obs_slot = h->d_obs_slot.p; P.tile_kf = h->d_tile_kf.p; P.tile_lmk = h->d_tile_lmk.p; P.tile_row = h->d_tile_row.p;
    P.pre_lane = h->plan.pre_ok ? (const int4*)h->d_pre_lane.p : nullptr; P.pre_kf = h->plan.pre_ok ? (const int2*)h->d_pre_kf.p : nullptr;
    P.ptab = h->d_ptab.p; P.ptab_stride = (long long)POSE_TAB * h->plan.n_kf_tot;
    P.priors = h->d_priors.p; P.prior_lin = h->d_prior_lin.p; P.prior_lin_stride = (long long)h->priors.size() * PRIOR_LIN; P.n_prior_tot = (int)h->priors.size();
    P.imus = h->d_imus.p; P.imu_scratch = h->d_imu_scratch.p; P.imu_scratch_stride = (long long)h->imus.size() * IMU_ROW;
    P.S = h->d_S.p; P.gred = h->d_gred.p; P.gfull = h->d_gfull.p; P.hdiag = h->d_hdiag.p;
    P.delta = h->d_delta.p; P.s_pose = h->d_s_pose.p;
    P.dbg_ts = h->d_dbg.p;
    P.trace = h->d_trace.p; P.t_start = h->d_tstart.p;
    P.states = h->d_states.p; P.acc = h->d_acc.p; P.tacc = h->d_tacc.p; P.n_tiles = (int)h->plan.tiles.size();
    P.state_stride = state_stride;
    P.final_out = h->h_final ? h->h_final : h->d_final.p;   // the final records go straight to pinned host memory (device-visible): no copy after the last kernel
    P.big_info = h->d_big_info.p;
    P.world = h->world; P.rank = h->rank; P.rank_b = h->d_rank_b.p; P.rank_s = h->d_rank_s.p;
    P.lmk_red = h->d_lmk_red.p; P.kept_obs = h->d_kept_obs.p; P.n_kept = h->plan.n_kept;
    P.dp_data = h->d_dp_data.p; P.dp_ints = h->d_dp_ints.p;
    P.sparse = h->d_sparse.p; P.sp_scratch = h->d_sp_scratch.p; P.sp_list = h->d_sp_list.p;
    P.sp_scratch_stride = (long long)std::max<size_t>(h->n_sparse_tot, 1) * SPARSE_J; P.n_imu_tot = (int)h->imus.size(); P.n_sp_list = h->n_sp_list;
    P.chunk_ob = h->d_chunk_ob.p; P.chunk_lm = h->d_chunk_lm.p; P.tile_perm = h->d_tile_perm.p; P.obs_lslot = h->d_obs_lslot.p;
    P.lm_hg = h->d_lm_hg.p; P.lm_hg_stride = (long long)LM_HG * std::max(h->plan.n_lmk_tot, 1);
    P.lm_dt = h->d_lm_dt.p; P.lm_dt_stride = (long long)LM_DT * std::max<long long>((long long)h->plan.tiles.size(), 1) * h->plan.lm_ksub;
    P.lm_sub = h->d_lm_sub.p; P.lm_ksub = h->plan.lm_ksub; P.lm_sub_per_item = h->plan.lm_sub_per_item; P.lm_sacc = h->plan.lm_ok ? h->d_lm_sacc.p : nullptr;
    P.lines = h->d_lines.p; P.lobs = h->d_lobs.p; P.xline = h->d_xline.p; P.line_scratch = h->d_line_scratch.p;
    P.xline_stride = 6LL * h->n_line_tot;
    P.n_xp = (long long)h->d_xp.n; P.n_xv = (long long)h->d_xv.n; P.n_xl = (long long)h->d_xl.n;
    P.n_win = (int)h->plan.wins.size();
    P.debug = h->env.debug;
    P.o = o;
    return P;
}
// Wide-panel factorisation (dense_chol.h): k_wchol_diag16 on the first 96 columns, then one k_wchol_step per further 96. The lower
// triangle of the N x N matrix A (leading dimension ld) is destroyed, y rides along as its right-hand side (-> L^-1 y). Lx (N x N,
// leading dimension ld): the panels below the diagonal blocks, out of place; Ltw: ceil(N / 96) * WD_LT doubles, the diagonal blocks'
// tiles; M: ceil(N / 96) 96 x 96 inverses of the diagonal blocks for k_wchol_backstep (null: factor only). dbg: phase stamps of the
// second k_wchol_step (SADVIO_DEBUG & 4096). Shared with marginalisation (marg_driver.h: run_wfac).
void launch_wfac(sadvio_ba_handle* h, double* A, long long ld, int N, double* y, double* Lx, double* Ltw, double* M, int* info, const int* skip, long long* dbg) {
    const int nsteps = (N + WD - 1) / WD;
    const size_t lds_d = sizeof(double) * wd16_lds_doubles() + 64, lds_st = sizeof(double) * wdstep_lds_doubles() + 64;
    (void)hipFuncSetAttribute((const void*)k_wchol_diag16, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds_d);
    (void)hipFuncSetAttribute((const void*)k_wchol_step, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds_st);
    hipLaunchKernelGGL(k_wchol_diag16, dim3(1), dim3(SOLVE_THREADS), lds_d, h->stream, A, ld, y, (double*)nullptr, N, 0, info, skip, Ltw);
    for (int st = 0; st + 1 < nsteps; st++) {
        const int c0 = st * WD, m = N - (c0 + WD);
        const int nt = (m + CH_TS - 1) / CH_TS;
        hipLaunchKernelGGL(k_wchol_step, dim3(nt * (nt + 1) / 2 + 2), dim3(SOLVE_THREADS), lds_st, h->stream, A, ld, Lx, y,
                           Ltw + (size_t)st * WD_LT, Ltw + (size_t)(st + 1) * WD_LT, M ? M + (size_t)st * WD * WD : nullptr,
                           M ? M + (size_t)(st + 1) * WD * WD : nullptr, N, c0, info, skip, st == 1 ? dbg : nullptr);
    }
}

// Rows below a block column of window w's S that can be non-zero, (hb + 1) * dpf: hb is the largest distance in free key-frame
// index that a landmark, an IMU pair or a relative-pose factor of the sparsified prior couples. N_p for a window whose reduced system
// keeps landmarks, carries a dense prior or has line landmarks (those fill S). One rule for the solve's band routes (plan_solve)
// and the covariance's (cov_driver.h). hb_out: hb, where the rule applies.
int window_bandwidth(const sadvio_ba_handle* h, int w, int* hb_out = nullptr) {
    const WinDev& d = h->plan.wins[w].d;
    int hb = h->plan.wins[w].hb_lmk;
    for (const ImuDev& f : h->imus_per_win[w]) {
        const int fi = h->plan.kf_fidx[f.kf_i], fj = h->plan.kf_fidx[f.kf_j];
        if (fi >= 0 && fj >= 0) hb = std::max(hb, std::abs(fi - fj));
    }
    if (w < (int)h->sparse_per_win.size())
        for (const sadvio_sparse_prior& sp : h->sparse_per_win[w])
            if (sp.type == SADVIO_SPARSE_RELATIVE_POSE) {     // a relative-pose factor couples its two key-frames
                const int fi = h->plan.kf_fidx[d.kf_base + sp.kf], fj = h->plan.kf_fidx[d.kf_base + sp.kf_b];
                if (fi >= 0 && fj >= 0) hb = std::max(hb, std::abs(fi - fj));
            }
    if (hb_out) *hb_out = hb;
    return (d.n_red > 0 || d.dp_n_full > 0 || d.line_end > d.line_begin) ? d.Np : std::min(d.Np, (hb + 1) * d.dpf);
}

// The reduced system of an out-of-LDS window (N_p > MAX_LDS_NP) is factored and solved in HBM by one of five routes (dense_chol.h),
// chosen once per solve call (BigPlan::choose).
enum class BigRoute {
    band,           // block-banded: one workgroup slides an LDS window down the band (k_band_solve)
    band_twisted,   // long band: the twisted factorisation, both ends at once (k_band_solve x 2 + k_band_mid)
    bcr,            // very long band of one window: block cyclic reduction over the bw x bw blocks (k_bcr_*)
    wide,           // not banded, N >= 2 * WD: 96-column panels on the matrix cores (launch_wfac + k_wchol_backstep)
    panel,          // not banded, N < 2 * WD: 32-column panels (k_chol_panel / k_chol_update / k_chol_backsolve)
};
// One per window, zeroed (memset) before it is filled: its bytes are part of the graph key. A window that fits LDS keeps ld == 0
// and nothing else of it is read.
struct BigPlan {
    BigRoute route;
    int bw;                       // rows below a block column of S that can be non-zero (block half-bandwidth + 1) * dpf
    int C;                        // band window of the band routes
    // Copies of the window's WinDev fields of the same names (plan_solve): the routes read these, never h->plan.wins, so that what they
    // launch with is keyed. A route that needs another WinDev field gets it here, not from the handle.
    int Np, ld, dpf, red_off;
    long long S_off;
    long long linv_off, mid_off, M_off, Lx_off;   // the window's share of d_big_linv / d_big_mid / d_big_M / d_big_Lx
    bool banded() const { return route == BigRoute::band || route == BigRoute::band_twisted || route == BigRoute::bcr; }
    // route and C from bw; on a sharded window bw is the all-reduced one, so every rank takes the same route
    void choose(int n_win, const EnvCfg& env) {
        const int N = Np, nb = dpf == 6 ? 6 : 5;
        if (!(bw < N && bw + nb <= MAX_LDS_NP)) {
            route = N >= 2 * WD ? BigRoute::wide : BigRoute::panel;
            return;
        }
        // with the update trimmed to the band a step costs the same in any window: the largest window that fits amortises the
        // per-window carry / load / store best (SADVIO_BAND_C overrides, for measurements)
        C = std::max(nb, (MAX_LDS_NP - bw) / nb * nb);
        if (env.band_c > 0) C = std::max(nb, std::min(C, env.band_c / nb * nb));
        const int Kb = (N + bw - 1) / bw;
        if (nb == 6 && Kb >= 22 && 2 * bw <= MAX_LDS_NP - 1 && n_win == 1 && !env.no_bcr) route = BigRoute::bcr;   // below ~22 blocks the twisted solver wins (measured)
        else if (N - bw >= 4 * C) route = BigRoute::band_twisted;
        else route = BigRoute::band;
    }
};

// The instantiations of a tile kernel template <FT, RARE, WITH_IMU, ONE>, indexed [one][pix][rare][with_imu] (FT 0 is the pixel factor). Only the plain
// variants exist with ONE (plan_solve never asks for another: those entries repeat the kernel without it).
#define SADVIO_TILE_VARIANTS(K) {{{{K<1, false, false>, K<1, false, true>}, {K<1, true, false>, K<1, true, true>}}, \
                                  {{K<0, false, false>, K<0, false, true>}, {K<0, true, false>, K<0, true, true>}}}, \
                                 {{{K<1, false, false, true>, K<1, false, true>}, {K<1, true, false>, K<1, true, true>}}, \
                                  {{K<0, false, false, true>, K<0, false, true>}, {K<0, true, false>, K<0, true, true>}}}}
using BuildFn = decltype(&k_build<0, false, false>);
using BacksubFn = decltype(&k_backsub<0, false, false>);
BuildFn build_variant(bool pix, bool rare, bool with_imu, bool one) {
    static const BuildFn t[2][2][2][2] = SADVIO_TILE_VARIANTS(k_build);
    return t[one][pix][rare][with_imu];
}
BacksubFn backsub_variant(bool pix, bool rare, bool with_imu, bool one) {
    static const BacksubFn t[2][2][2][2] = SADVIO_TILE_VARIANTS(k_backsub);
    return t[one][pix][rare][with_imu];
}
#undef SADVIO_TILE_VARIANTS

// Everything the per-slot launch sequence reads, decided before any launch (plan_solve). Zeroed (memset) before it is filled, so
// that two plans with equal fields are equal bytes: with the BigPlan of every window it is the key of the captured graph.
struct SolvePlan {
    DevPtrs P;             // kernel argument; also holds n_win, n_tiles, n_kept, state_stride (= slots + 2), decide_kernel, world
    int slots;             // step attempts enqueued
    int mtk, Rp, strip_doubles;
    int n_kf_tot, n_pf, n_lo, dp_max_nf, dp_max_n, reset_blocks, table_blocks, max_win_tiles, lm_n_sub, lm_sub_obs, n_big;
    bool pix, rare, with_imu, use_lm, extras, fork;
    bool one_round;        // the tile kernels are the ONE instantiations (k_build / k_backsub without the loop over landmark rounds)
    bool coll_band;        // sharded: only the band of the one window's S travels (coll_buf = the packed copy)
    size_t lds_build, lds_back, lds_solve, lds_bobs, lds_pass0, lds_pass, lds_long_lin, lds_long_back;
    BuildFn k_build;
    BacksubFn k_backsub;
    decltype(&k_build_kept<0>) k_build_kept;
    decltype(&k_build_obs<0>) k_build_obs;
    LongArgs lg;                              // long tracks (long_kernels.h): their kernels are launched when lg.n_long > 0
    decltype(&k_long_lin<0>) k_long_lin;
    decltype(&k_long_back<0>) k_long_back;
    decltype(&k_lm_pass<0, false>) k_lm_pass, k_lm_pass0;
    decltype(&k_solve<0, false>) k_solve, k_solve_front, k_solve_back;
    // workspaces of the out-of-LDS routes. They are part of the key in their own right: a workspace that grows moves, and a graph
    // captured with the old address must not be replayed
    double *big_linv, *big_mid, *big_M, *big_Lx, *bcr;
    double* coll_buf;      // sharded: what the per-slot all-reduce of the reduced system sends, coll_count doubles
    long long coll_count;
};
static_assert(std::is_trivially_copyable<SolvePlan>::value && std::is_trivially_copyable<BigPlan>::value, "the graph key is their bytes");

// LDS of the band kernels (k_band_solve, k_band_mid, k_bcr_elim / root): the in-LDS solver's window of R rows (pivot strip, packed
// triangle + rhs row, two vectors) and `blocks` inverse pivot blocks of nb x nb
size_t band_lds_bytes(int R, int nb, int blocks) {
    return sizeof(double) * ((size_t)(R + 2) * 6 + (size_t)(R + 1) * (R + 2) / 2 + 2 * (size_t)R + (size_t)blocks * nb * nb) + 64;
}

// The routes: S (leading dimension p.ld) and y = gred of the window in place; dbg: SADVIO_DEBUG & 4096 stamps of this slot
void solve_band(sadvio_ba_handle* h, const SolvePlan& pl, const BigPlan& p, double* S, double* y, int* info, const int* skip, bool dbg) {
    const int N = p.Np, bw = p.bw, C = p.C, nb = p.dpf == 6 ? 6 : 5;
    const int Rmax = bw + C;
    const size_t lds = band_lds_bytes(Rmax, nb, Rmax / nb + 1);
    auto kbs = p.dpf == 6 ? k_band_solve<6> : k_band_solve<5>;
    (void)hipFuncSetAttribute((const void*)kbs, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
    long long* ts = dbg ? pl.P.dbg_ts + 44 : nullptr;
    double* lv = pl.big_linv + p.linv_off;
    if (p.route == BigRoute::band) {
        hipLaunchKernelGGL(kbs, dim3(1), dim3(SOLVE_THREADS), lds, h->stream, S, (long long)p.ld, y, lv, N, bw, C, info, skip, ts, -1, 0, (double*)nullptr);
        return;
    }
    const int M = (N - bw) / 2 / nb * nb;
    double* md = pl.big_mid + p.mid_off;
    auto kbm = p.dpf == 6 ? k_band_mid<6> : k_band_mid<5>;
    const size_t lds_m = band_lds_bytes(bw, nb, bw / nb + 1);
    (void)hipFuncSetAttribute((const void*)kbm, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds_m);
    if (dbg) fprintf(stderr, "[sadvio dbg] twisted band solve N %d bw %d C %d M %d\n", N, bw, C, M);
    hipLaunchKernelGGL(kbs, dim3(2), dim3(SOLVE_THREADS), lds, h->stream, S, (long long)p.ld, y, lv, N, bw, C, info, skip, ts, M, 0, md);
    hipLaunchKernelGGL(kbm, dim3(1), dim3(SOLVE_THREADS), lds_m, h->stream, S, (long long)p.ld, y, N, bw, M, md, info, skip);
    hipLaunchKernelGGL(kbs, dim3(2), dim3(SOLVE_THREADS), lds, h->stream, S, (long long)p.ld, y, lv, N, bw, C, info, skip, ts, M, 1, md);
}

size_t bcr_doubles(int N, int bw) {
    const size_t b = (size_t)bw, K = ((size_t)N + b - 1) / b;
    return K * (8 * b * b + b * (b + 1) / 2 + (b / 6) * 36 + 5 * b);
}

void solve_bcr(sadvio_ba_handle* h, const SolvePlan& pl, const BigPlan& p, double* S, double* y, int* info, const int* skip, bool dbg) {
    const int N = p.Np, bw = p.bw, Kb = (N + bw - 1) / bw;
    const size_t b = (size_t)bw, bb = b * b, K = (size_t)Kb;
    BcrPtrs B{};
    double* q = pl.bcr;
    B.D = q; q += K * bb; B.E = q; q += K * bb; B.Wp = q; q += K * bb; B.Wn = q; q += K * bb;
    B.Ul = q; q += K * bb; B.Ur = q; q += K * bb;
    B.Lp = q; q += K * (b * (b + 1) / 2); B.linv = q; q += K * (b / 6) * 36;
    B.g = q; q += K * b; B.yv = q; q += K * b; B.gl = q; q += K * b; B.gr = q; q += K * b; B.X = q; q += K * b;
    B.K = Kb; B.b = bw; B.N = N;
    const size_t lds_e = band_lds_bytes(2 * bw, 6, bw / 6 + 1);
    const size_t lds_c = sizeof(double) * 2 * b * (b + 1);
    const size_t lds_r = band_lds_bytes(2 * bw, 6, 2 * (bw / 6 + 1));   // up to two blocks, all 2 b / 6 pivot blocks kept
    const size_t lds_b = sizeof(double) * (b * (b + 1) / 2 + 4 * b + (b / 6) * 36);
    (void)hipFuncSetAttribute((const void*)k_bcr_elim<6>, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds_e);
    (void)hipFuncSetAttribute((const void*)k_bcr_combine, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds_c);
    (void)hipFuncSetAttribute((const void*)k_bcr_root<6>, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds_r);
    (void)hipFuncSetAttribute((const void*)k_bcr_back<6>, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds_b);
    hipLaunchKernelGGL(k_bcr_extract, dim3(Kb), dim3(256), 0, h->stream, S, (long long)p.ld, y, B, skip, info);
    int smax = 0, s_root = 0;
    for (int sst = 1; sst < Kb; sst *= 2) {
        const int na = (Kb + sst - 1) / sst;
        if (na == 2) { s_root = sst; break; }   // two blocks left: solved together by k_bcr_root
        hipLaunchKernelGGL(k_bcr_elim<6>, dim3(na / 2, 2), dim3(SOLVE_THREADS), lds_e, h->stream, B, sst, info, skip);
        hipLaunchKernelGGL(k_bcr_combine, dim3(na), dim3(512), lds_c, h->stream, B, sst, info, skip);
        smax = sst;
    }
    hipLaunchKernelGGL(k_bcr_root<6>, dim3(1), dim3(SOLVE_THREADS), lds_r, h->stream, B, s_root, info, skip);
    for (int sst = smax; sst >= 1; sst /= 2) {
        const int na = (Kb + sst - 1) / sst;
        hipLaunchKernelGGL(k_bcr_back<6>, dim3(na / 2), dim3(256), lds_b, h->stream, B, sst, info, skip);
    }
    hipLaunchKernelGGL(k_bcr_writeback, dim3((N + 255) / 256), dim3(256), 0, h->stream, B, y, info, skip);
    if (dbg) fprintf(stderr, "[sadvio dbg] block cyclic reduction N %d bw %d K %d\n", N, bw, Kb);
}

void solve_wide(sadvio_ba_handle* h, const SolvePlan& pl, const BigPlan& p, double* S, double* y, int* info, const int* skip, bool dbg) {
    const int N = p.Np, nsteps = (N + WD - 1) / WD;
    double* M = pl.big_M + p.M_off;
    double* Ltw = M + (size_t)nsteps * WD * WD;
    (void)hipFuncSetAttribute((const void*)k_wchol_backstep, hipFuncAttributeMaxDynamicSharedMemorySize, (int)(sizeof(double) * WD * WDS));
    launch_wfac(h, S, (long long)p.ld, N, y, pl.big_Lx + p.Lx_off, Ltw, M, info, skip, dbg ? pl.P.dbg_ts + 106 : nullptr);
    for (int bs = nsteps - 1; bs >= 0; bs--)
        hipLaunchKernelGGL(k_wchol_backstep, dim3(1 + (bs + 1 < nsteps ? (bs * WD + 63) / 64 : 0)), dim3(SOLVE_THREADS), sizeof(double) * WD * WDS, h->stream,
                           pl.big_Lx + p.Lx_off, (long long)p.ld, y, M, N, bs, info, skip);
}

void solve_panel(sadvio_ba_handle* h, const SolvePlan& pl, const BigPlan& p, double* S, double* y, int* info, const int* skip, bool dbg) {
    const int N = p.Np;
    for (int k0 = 0; k0 < N; k0 += CH_NB) {
        const int nb = std::min(CH_NB, N - k0), s0 = k0 + nb;
        const int rows_end = std::min(N, s0 + p.bw), m = rows_end - s0;
        hipLaunchKernelGGL(k_chol_panel, dim3((m + 1 + CH_THREADS - 1) / CH_THREADS), dim3(CH_THREADS), 0, h->stream,
                           S, (long long)p.ld, y, N, k0, rows_end, info, skip, dbg && k0 == 64 ? pl.P.dbg_ts + 44 : nullptr);
        if (m > 0) {
            const int nt = (m + CH_TS - 1) / CH_TS;
            hipLaunchKernelGGL(k_chol_update, dim3(nt * (nt + 1) / 2 + (m + CH_THREADS - 1) / CH_THREADS), dim3(CH_THREADS), 0,
                               h->stream, S, (long long)p.ld, y, N, k0, rows_end, info, skip);
        }
    }
    hipLaunchKernelGGL(k_chol_backsolve, dim3(1), dim3(CH_THREADS), 0, h->stream, S, (long long)p.ld, y, N, p.bw, info, skip);
}

// Cholesky + solve of the reduced system of out-of-LDS window w at slot s by the route of its plan
void solve_big(sadvio_ba_handle* h, const SolvePlan& pl, const BigPlan& p, int w, int s, bool dbg) {
    double* S = pl.P.S + p.S_off;
    double* y = pl.P.gred + p.red_off;
    int* info = pl.P.big_info + w;
    const int* skip = (const int*)((const char*)(pl.P.states + (size_t)w * pl.P.state_stride + s) + offsetof(LmState, done));
    switch (p.route) {
        case BigRoute::band: case BigRoute::band_twisted: solve_band(h, pl, p, S, y, info, skip, dbg); break;
        case BigRoute::bcr: solve_bcr(h, pl, p, S, y, info, skip, dbg); break;
        case BigRoute::wide: solve_wide(h, pl, p, S, y, info, skip, dbg); break;
        case BigRoute::panel: solve_panel(h, pl, p, S, y, info, skip, dbg); break;
    }
}

// Decide one solve: state and workspace allocations, launch parameters, kernel variants, the route of every out-of-LDS window.
int plan_solve(sadvio_ba_handle* h, const SolveOpts& o, SolvePlan& plan, std::vector<BigPlan>& big) {
    memset(&plan, 0, sizeof(plan));
    const int n_win = (int)h->plan.wins.size();
    // Slot s (s = 0 .. slots-1) is one step attempt; with max_num_iterations = 0 Ceres still evaluates
    // iteration 0, so at least one slot is always run and the final decision is taken by k_final.
    const int slots = plan.slots = std::max(1, o.max_num_iterations);
    const int stride = slots + 2;
    HIP_TRY(h->d_dbg.alloc(DBG_SLOTS));
    HIP_TRY(h->d_states.alloc((size_t)n_win * stride));
    HIP_TRY(h->d_trace.alloc((size_t)n_win * stride * 8));
    HIP_TRY(h->d_tstart.alloc(1));
    HIP_TRY(h->d_acc.alloc((size_t)n_win * stride));
    HIP_TRY(h->d_final.alloc((size_t)n_win));
    HIP_TRY(h->d_big_info.alloc((size_t)n_win));
    if (h->h_final_n < (size_t)n_win) {
        if (h->h_final) (void)hipHostFree(h->h_final);
        h->h_final = nullptr; h->h_final_n = 0;
        HIP_TRY(hipHostMalloc((void**)&h->h_final, sizeof(FinalRec) * (size_t)n_win, hipHostMallocDefault));
        h->h_final_n = (size_t)n_win;
    }
    DevPtrs& P = plan.P;
    P = make_ptrs(h, o, stride);
    const int n_tiles = (int)h->plan.tiles.size();
    // with many tiles, re-summing all partials in every k_build workgroup costs more than one tiny launch per slot
    // The decision of a slot is re-derived by every k_build workgroup from its OWN window's tile partials (read by all 256 threads
    // with every load in flight: the cost does not depend on how many windows the batch has), as long as a window has at most
    // 4 * BUILD_THREADS tiles (the canonical summation order of wave_sum_backsub_partials); a separate k_decide launch per slot
    // only for larger windows (configs 4 / 5) and for the throughput kernels, which read the decided state.
    int max_win_tiles = 0;
    for (int w = 0; w < n_win; w++) max_win_tiles = std::max(max_win_tiles, h->plan.wins[w].d.tile_end - h->plan.wins[w].d.tile_begin);
    plan.max_win_tiles = max_win_tiles;
    P.decide_kernel = max_win_tiles > 4 * BUILD_THREADS ? 1 : 0;
    P.c16_old_tail = h->env.c16_old_tail ? 1 : 0;
    // a sharded window keeps the item loop of k_solve: every rank must leave it with the same bits (plain adds, one factor at a time)
    P.imu_direct = (!h->coll_fn && P.world == 1 && !h->env.imu_items) ? 1 : 0;
    const int mtk = plan.mtk = h->plan.max_tile_kf;
    const size_t nt = 6 * (size_t)h->plan.max_tile_free;
    int Rp = 16 * ((6 * h->plan.max_gemm_free + 15) / 16);                          // padded rows of the Y / E strips
    int strip_doubles = std::max(STAGE_VALS * 64, 2 * Rp * (32 + 2));          // per wave: Y | E strips, later the wave's copy of the tile
    size_t lds_build = tile_tables_bytes(mtk) + sizeof(double) * ((size_t)BUILD_WAVES * strip_doubles + nt * (nt + 1) / 2 + 3 * nt +
                                                                   0) + 16;
    if (lds_build > 160 * 1024 && h->plan.max_gemm_free > 0) {
        // a window mixing short tracks with very long ones: the MFMA strips + the large atomic tile do not fit
        // together; run every tile on the ds_add_f64 path instead. This is the only write to the layout a solve makes
        for (auto& t : h->plan.tiles) if (t.lds_mode == 2) t.lds_mode = 1;
        HIP_TRY(hipMemcpyAsync(h->d_tiles.p, h->plan.tiles.data(), h->plan.tiles.size() * sizeof(Tile), hipMemcpyHostToDevice, h->stream));
        h->plan.max_gemm_free = 0;
        Rp = 0; strip_doubles = STAGE_VALS * 64;
        lds_build = tile_tables_bytes(mtk) + sizeof(double) * ((size_t)BUILD_WAVES * strip_doubles + nt * (nt + 1) / 2 + 3 * nt +
                                                               0) + 16;
    }
    if (h->env.debug) fprintf(stderr, "[sadvio dbg] lds_build %zu B, Rp %d, strip_doubles %d, max_tile_kf %d, max_tile_free %d, tiles %d\n", lds_build, Rp, strip_doubles, mtk, h->plan.max_tile_free, n_tiles);
    plan.Rp = Rp; plan.strip_doubles = strip_doubles; plan.lds_build = lds_build;
    plan.lds_back = tile_tables_bytes(mtk) + sizeof(double) * ((size_t)mtk * 18) + 16;
    // k_solve<0>: tile-packed image + y / gf / hd / xs + the chol16 exchange areas
    const size_t npq = (size_t)h->plan.max_np;
    plan.lds_solve = sizeof(double) * ((size_t)c16_size((int)npq) + 4 * npq + 1 + C16_WORK + 16 * (size_t)c16_blocks((int)npq + 1) + SOLVE_KFC * SOLVE_KFC_STRIDE) + 64;
    // robust loss or prior-kept landmarks in the batch: the kernels carrying those (rare) paths
    bool any_pseudo = false;
    for (const auto& v : h->plan.sp_elim) for (char e : v) any_pseudo |= e != 0;
    // (kept landmarks: by their reduced columns, not by their observations — on a sharded window the ranks other than 0 hold them without any)
    bool any_kept_lmk = false;
    for (int w = 0; w < n_win; w++) any_kept_lmk |= h->plan.wins[w].d.n_red > 0;
    const bool rare = plan.rare = o.huber_a > 0.0 || h->plan.n_kept > 0 || any_kept_lmk || any_pseudo || h->plan.gemm_run4;
    const bool pix = plan.pix = h->plan.factor_type == SADVIO_FACTOR_PIXEL;
    // IMU factor pairs and listed sparse-prior factors ride k_build (linearisation) and k_backsub (candidate cost) as extra workgroups
    // when the submission is a window or two: the inlined linearisation leaves those variants of k_build one workgroup per CU, which
    // a batch of VIO windows would pay for; there the evaluation runs as kernels of its own on the same stream (k_pf_eval)
    const bool have_pf = !h->imus.empty() || h->n_sp_list > 0;
    bool with_imu = have_pf && n_tiles <= 3 * 256;
    if (h->env.pf_wg >= 0) with_imu = have_pf && h->env.pf_wg != 0;
    plan.with_imu = with_imu;
    // Single-round tiles (a single window, a small batch) on the plain kernels: the instantiations without the loop over landmark rounds.
    // SADVIO_NO_ONE_ROUND=1 keeps the looping kernels (A/B, tests); it reaches the graph key through this field.
    const bool one = plan.one_round = h->plan.single_round && !rare && !with_imu && !h->env.no_one_round;
    plan.k_build = build_variant(pix, rare, with_imu, one);
    plan.k_backsub = backsub_variant(pix, rare, with_imu, one);
    plan.k_build_kept = pix ? k_build_kept<0> : k_build_kept<1>;
    if (h->plan.n_long > 0) {
        plan.lg.n_long = h->plan.n_long; plan.lg.max_kf = h->plan.long_max_kf;
        plan.lg.rec = h->d_long_rec.p; plan.lg.kf = h->d_long_kf.p; plan.lg.slot = h->d_long_slot.p;
        plan.k_long_lin = pix ? k_long_lin<0> : k_long_lin<1>;
        plan.k_long_back = pix ? k_long_back<0> : k_long_back<1>;
        plan.lds_long_lin = long_lds_bytes(plan.lg.max_kf); plan.lds_long_back = long_lds_bytes(0);
        HIP_TRY(hipFuncSetAttribute((const void*)plan.k_long_lin, hipFuncAttributeMaxDynamicSharedMemorySize, (int)plan.lds_long_lin));
    }
    // large plain batches: the throughput kernels of lm_kernels.h (SADVIO_LM=1 / 0 forces / forbids them, for tests and A/B runs)
    bool use_lm = h->plan.lm_ok && !rare && !h->coll_fn && h->world == 1 && h->plan.lm_landmarks >= 65536;
    if (h->env.lm >= 0) use_lm = h->plan.lm_ok && !rare && !h->coll_fn && h->world == 1 && h->env.lm != 0;
    plan.use_lm = use_lm;
    plan.k_build_obs = pix ? k_build_obs<0> : k_build_obs<1>;
    plan.k_lm_pass = pix ? k_lm_pass<0, false> : k_lm_pass<1, false>;
    plan.k_lm_pass0 = pix ? k_lm_pass<0, true> : k_lm_pass<1, true>;
    plan.lm_n_sub = h->plan.lm_n_sub; plan.lm_sub_obs = h->plan.lm_sub_obs;
    const size_t lds_views = pix ? sizeof(double) * (size_t)mtk * h->plan.lm_max_cam * LM_VT : 0;   // view tables of the pixel factor
    plan.lds_bobs = tile_tables_bytes(mtk) + sizeof(double) * ((size_t)BUILD_WAVES * Rp * LM_KS + nt * (nt + 1) / 2 + nt + 1 + LM_DT) + lds_views + 16;
    // k_lm_pass: tables at x (+ at the candidate, + the pose steps), the tile's key-frame sums, the staged observation constants
    plan.lds_pass0 = tile_tables_bytes(mtk) + sizeof(double) * LM_DT_COST + (size_t)h->plan.lm_sub_obs * ((pix ? 2 : 3) * sizeof(double) + sizeof(int)) + lds_views + 16;
    plan.lds_pass = plan.lds_pass0 + sizeof(double) * (size_t)mtk * (POSE_TAB + 6) + lds_views;
    if (!use_lm) P.lm_sacc = nullptr;   // k_decide sums the tiles' k_backsub partials
    if (use_lm) {
        P.decide_kernel = 1;   // the kernels read the decided state of their slot
        HIP_TRY(hipFuncSetAttribute((const void*)plan.k_build_obs, hipFuncAttributeMaxDynamicSharedMemorySize, (int)plan.lds_bobs));
        HIP_TRY(hipFuncSetAttribute((const void*)plan.k_lm_pass, hipFuncAttributeMaxDynamicSharedMemorySize, (int)plan.lds_pass));
        HIP_TRY(hipFuncSetAttribute((const void*)plan.k_lm_pass0, hipFuncAttributeMaxDynamicSharedMemorySize, (int)plan.lds_pass0));
    }
    HIP_TRY(hipFuncSetAttribute((const void*)plan.k_build, hipFuncAttributeMaxDynamicSharedMemorySize, (int)plan.lds_build));
    HIP_TRY(hipFuncSetAttribute((const void*)plan.k_backsub, hipFuncAttributeMaxDynamicSharedMemorySize, (int)plan.lds_back));
    bool extras = false;  // any pose-only factor family beyond PosePriordx in the batch?
    for (int w = 0; w < n_win; w++) {
        const WinDev& d = h->plan.wins[w].d;
        if (d.imu_end > d.imu_begin || d.sp_end > d.sp_begin || d.dp_n_full > 0 || d.dpf == 15 || d.lobs_end > d.lobs_begin || d.line_end > d.line_begin) extras = true;   // dpf 15: padded pivots live in the EXTRAS kernel
    }
    plan.extras = extras;
    plan.k_solve = extras ? k_solve<0, true> : k_solve<0, false>;
    plan.k_solve_front = extras ? k_solve<1, true> : k_solve<1, false>;
    plan.k_solve_back = extras ? k_solve<2, true> : k_solve<2, false>;
    HIP_TRY(hipFuncSetAttribute((const void*)plan.k_solve, hipFuncAttributeMaxDynamicSharedMemorySize, (int)plan.lds_solve));
    plan.n_kf_tot = h->plan.n_kf_tot; plan.n_big = h->plan.n_big;
    plan.reset_blocks = (int)std::min<long long>(1024, std::max<long long>(1, (P.n_xl + P.n_xp + 255) / 256));
    // (extra blocks of k_reset) the pose tables / prior records at x = 0
    plan.table_blocks = (std::max(h->plan.n_kf_tot, (int)h->priors.size()) + 63) / 64;
    // IMU factor pairs and the listed sparse-prior factors ride the tile kernels as extra workgroups (kernels.h: pose_factor_eval).
    // Line observations are still evaluated on a side stream: the linearisation next to k_build, the candidate cost next to
    // k_backsub (fork / join with events; parallel branches of the captured graph)
    plan.n_pf = (int)h->imus.size() + h->n_sp_list;
    plan.n_lo = h->n_lobs_tot;
    plan.fork = plan.n_lo > 0 && h->side && !h->cfg.profile_kernels && !h->coll_fn && !h->env.no_fork;
    // rows below a block column of S that can be non-zero: (block half-bandwidth + 1) * dpf from the co-visibility
    // structure and the IMU pairs; a dense prior fills the kept-landmark block, so those windows are dense
    big.clear(); big.resize(n_win);
    if (n_win) memset(big.data(), 0, sizeof(BigPlan) * (size_t)n_win);
    for (int w = 0; w < n_win; w++) {
        const WinDev& d = h->plan.wins[w].d;
        if (!d.ld) continue;
        BigPlan& p = big[w];
        p.Np = d.Np; p.ld = d.ld; p.dpf = d.dpf; p.red_off = d.red_off; p.S_off = d.S_off;
        p.bw = window_bandwidth(h, w);
    }
    if (h->coll_fn && h->world > 1 && h->plan.n_big) {
        // every rank must factor the all-reduced S with the same (largest) bandwidth: gather the local ones
        std::vector<double> slots((size_t)n_win * h->world * 4, 0.0);
        for (int w = 0; w < n_win; w++) slots[((size_t)w * h->world + h->rank) * 4] = (double)big[w].bw;
        HIP_TRY(hipMemcpyAsync(h->d_rank_s.p, slots.data(), slots.size() * sizeof(double), hipMemcpyHostToDevice, h->stream));
        if (h->coll_fn(h->coll_ctx, h->d_rank_s.p, (int64_t)slots.size(), (void*)h->stream) != 0) { h->err = "solve: all-reduce failed"; return SADVIO_E_RCCL; }
        HIP_TRY(hipMemcpyAsync(slots.data(), h->d_rank_s.p, slots.size() * sizeof(double), hipMemcpyDeviceToHost, h->stream));
        HIP_TRY(hipStreamSynchronize(h->stream));
        for (int w = 0; w < n_win; w++)
            for (int r = 0; r < h->world; r++) big[w].bw = std::max(big[w].bw, (int)slots[((size_t)w * h->world + r) * 4]);
    }
    {
        // the route of every out-of-LDS window and the workspace it needs, allocated here, never inside the (possibly captured) launch sequence
        long long totv = 0, totm = 0, totM = 0, totL = 0;
        for (int w = 0; w < n_win; w++) {
            BigPlan& p = big[w];
            if (!p.ld) continue;
            p.choose(n_win, h->env);
            const long long b = p.bw;
            if (p.route == BigRoute::band || p.route == BigRoute::band_twisted) { p.linv_off = totv; totv += 6LL * p.Np; }
            if (p.route == BigRoute::band_twisted) { p.mid_off = totm; totm += 2 * (b * (b + 1) / 2 + b); }
            if (p.route == BigRoute::bcr) HIP_TRY(h->d_bcr.alloc(bcr_doubles(p.Np, p.bw)));   // (one window only)
            if (p.route == BigRoute::wide) {
                p.M_off = totM; totM += (long long)((p.Np + WD - 1) / WD) * (WD * WD + WD_LT);   // M | the factors' tiles
                p.Lx_off = totL; totL += (long long)p.Np * p.ld;                              // the out-of-place panels
            }
        }
        HIP_TRY(h->d_big_linv.alloc((size_t)std::max<long long>(totv, 1)));
        HIP_TRY(h->d_big_mid.alloc((size_t)std::max<long long>(totm, 1)));
        HIP_TRY(h->d_big_M.alloc((size_t)std::max<long long>(totM, 1)));
        HIP_TRY(h->d_big_Lx.alloc((size_t)std::max<long long>(totL, 1)));
        plan.big_linv = h->d_big_linv.p; plan.big_mid = h->d_big_mid.p; plan.big_M = h->d_big_M.p; plan.big_Lx = h->d_big_Lx.p; plan.bcr = h->d_bcr.p;
    }
    if (h->coll_fn) {
        // the window spans devices: what the per-slot all-reduce of the reduced system sends
        plan.coll_buf = h->d_S.p; plan.coll_count = h->plan.red_total;
        if (n_win == 1 && big[0].ld && big[0].bw < big[0].Np && big[0].S_off == 0) {
            // one banded window spanning the devices: only the band of S travels (dense_chol.h: k_band_pack)
            const long long nbd = (long long)big[0].Np * big[0].bw, tail = h->plan.red_total - (long long)big[0].Np * big[0].ld;
            HIP_TRY(h->d_coll_band.alloc((size_t)(nbd + tail)));
            plan.coll_band = true; plan.coll_buf = h->d_coll_band.p; plan.coll_count = nbd + tail;
        }
    }
    for (int w = 0; w < n_win; w++) { plan.dp_max_nf = std::max(plan.dp_max_nf, h->plan.wins[w].d.dp_n_full); plan.dp_max_n = std::max(plan.dp_max_n, h->plan.wins[w].d.dp_n); }
    return SADVIO_OK;
}

// The launch sequence of one solve (all slots) on the handle's stream(s), possibly under stream capture. Launch geometry, LDS sizes,
// flags, counts and device pointers come from the plan alone; the handle gives the streams and events, the kernel timers and the
// collective hook. Returns false when a collective failed.
bool enqueue_solve(sadvio_ba_handle* h, const SolvePlan& pl, const std::vector<BigPlan>& big) {
    const DevPtrs& P = pl.P;
    const int n_win = P.n_win, n_tiles = P.n_tiles, n_kept = P.n_kept, mtk = pl.mtk, n_pf = pl.n_pf, n_lo = pl.n_lo;
    const bool fork = pl.fork, use_lm = pl.use_lm, with_imu = pl.with_imu;
    bool coll_ok = true;
    {   // zero deltas / accumulators + initial LM state, and (extra blocks) the pose tables / prior records at x = 0
        ScopedTimer t(h, "k_reset");
        hipLaunchKernelGGL(k_reset, dim3(pl.reset_blocks + pl.table_blocks), dim3(256), 0, h->stream, P, pl.reset_blocks, pl.n_kf_tot);
    }
    for (int s = 0; s < pl.slots; s++) {
        if (fork) {
            (void)hipEventRecord(h->ev_fork, h->stream);
            (void)hipStreamWaitEvent(h->side, h->ev_fork, 0);
            if (n_lo) hipLaunchKernelGGL(k_line_eval<true>, dim3(n_lo), dim3(64), 0, h->side, P, s, 1);
            (void)hipEventRecord(h->ev_lin, h->side);
        }
        if (use_lm) {
            // the opening pass linearises at x (H_ll, g_l per landmark, key-frame sums per tile); later slots get them from the
            // candidate pass of the slot before
            if (s == 0) { ScopedTimer t(h, "k_lm_pass0"); hipLaunchKernelGGL(pl.k_lm_pass0, dim3(pl.lm_n_sub), dim3(LM_PASS_THREADS), pl.lds_pass0, h->stream, P, s, mtk, pl.lm_sub_obs); }
            { ScopedTimer t(h, "k_build_obs"); hipLaunchKernelGGL(pl.k_build_obs, dim3(n_tiles), dim3(BUILD_THREADS), pl.lds_bobs, h->stream, P, s, mtk, pl.Rp); }
        } else
        { ScopedTimer t(h, "k_build"); hipLaunchKernelGGL(pl.k_build, dim3(n_tiles + (with_imu ? n_pf : 0)), dim3(BUILD_THREADS), pl.lds_build, h->stream, P, s, mtk, pl.strip_doubles, pl.Rp); }
        if (n_pf && (use_lm || !with_imu)) { ScopedTimer t(h, "k_pf_lin"); hipLaunchKernelGGL(k_pf_eval<false>, dim3(n_pf), dim3(BUILD_THREADS), 0, h->stream, P, s); }
        if (n_kept) { ScopedTimer t(h, "k_build_kept"); hipLaunchKernelGGL(pl.k_build_kept, dim3((n_kept + 127) / 128), dim3(128), 0, h->stream, P, s); }
        if (pl.lg.n_long) { ScopedTimer t(h, "k_long_lin"); hipLaunchKernelGGL(pl.k_long_lin, dim3(pl.lg.n_long), dim3(LONG_THREADS), pl.lds_long_lin, h->stream, P, pl.lg, s); }
        if (pl.dp_max_nf > 0) {
            ScopedTimer t(h, "k_prior_r+gh");
            const int colb = (pl.dp_max_n + 3) / 4;
            hipLaunchKernelGGL(k_prior_r, dim3((pl.dp_max_nf + 3) / 4, n_win), dim3(256), 0, h->stream, P, s);
            hipLaunchKernelGGL(k_prior_gh, dim3(colb + (unsigned)(((long long)pl.dp_max_n * pl.dp_max_n + 255) / 256), n_win), dim3(256), 0, h->stream, P, s, colb);
        }
        if (h->coll_fn) {
            // the window spans devices: gather the per-rank partial sums and all-reduce the reduced system
            { ScopedTimer t(h, "k_rank_partials"); hipLaunchKernelGGL(k_rank_partials, dim3(n_win), dim3(64), 0, h->stream, P, s, 0); }
            ScopedTimer t(h, "allreduce_reduced_system");
            if (pl.coll_band) {
                // one banded window spanning the devices: only the band of S travels (dense_chol.h: k_band_pack)
                const BigPlan& b0 = big[0];
                const long long nbd = (long long)b0.Np * b0.bw, tail = pl.coll_count - nbd;
                const int pb = (int)std::min<long long>((nbd + tail + 255) / 256, 2048);
                hipLaunchKernelGGL(k_band_pack, dim3(pb), dim3(256), 0, h->stream, P.S, (long long)b0.ld, b0.Np, b0.bw, tail, pl.coll_buf, 0);
                if (h->coll_fn(h->coll_ctx, pl.coll_buf, (int64_t)pl.coll_count, (void*)h->stream) != 0) coll_ok = false;
                hipLaunchKernelGGL(k_band_pack, dim3(pb), dim3(256), 0, h->stream, P.S, (long long)b0.ld, b0.Np, b0.bw, tail, pl.coll_buf, 1);
            } else if (h->coll_fn(h->coll_ctx, pl.coll_buf, (int64_t)pl.coll_count, (void*)h->stream) != 0) coll_ok = false;
        }
        if (fork) (void)hipStreamWaitEvent(h->stream, h->ev_lin, 0);
        else {
            if (n_lo) { ScopedTimer t(h, "k_line_lin"); hipLaunchKernelGGL(k_line_eval<true>, dim3(n_lo), dim3(64), 0, h->stream, P, s, 0); }
        }
        if (pl.n_big < n_win) { ScopedTimer t(h, "k_solve"); hipLaunchKernelGGL(pl.k_solve, dim3(n_win), dim3(SOLVE_THREADS), pl.lds_solve, h->stream, P, s); }
        if (pl.n_big) {
            { ScopedTimer t(h, "k_solve_front"); hipLaunchKernelGGL(pl.k_solve_front, dim3(n_win), dim3(SOLVE_THREADS), 64, h->stream, P, s); }
            {
                ScopedTimer t(h, "reduced_cholesky_solve");
                for (int w = 0; w < n_win; w++)
                    if (big[w].ld) solve_big(h, pl, big[w], w, s, (P.debug & 4096) && s == 3);
            }
            { ScopedTimer t(h, "k_solve_back"); hipLaunchKernelGGL(pl.k_solve_back, dim3(n_win), dim3(SOLVE_THREADS), 64, h->stream, P, s); }
            for (int w = 0; w < n_win; w++) {
                const BigPlan& p = big[w];
                if (!p.ld) continue;
                if (p.banded())   // only the band was written
                    hipLaunchKernelGGL(k_band_zero, dim3((unsigned)std::min<long long>(((long long)p.Np * p.bw + 255) / 256, 4096)), dim3(256), 0, h->stream,
                                       P.S + p.S_off, (long long)p.ld, p.Np, p.bw);
                else (void)hipMemsetAsync(P.S + p.S_off, 0, sizeof(double) * (size_t)p.Np * p.Np, h->stream);
            }
        }
        if (fork) {
            (void)hipEventRecord(h->ev_solved, h->stream);
            (void)hipStreamWaitEvent(h->side, h->ev_solved, 0);
            if (n_lo) hipLaunchKernelGGL(k_line_eval<false>, dim3(n_lo), dim3(64), 0, h->side, P, s, 0);
            (void)hipEventRecord(h->ev_cost, h->side);
        } else {
            if (n_lo) { ScopedTimer t(h, "k_line_cost"); hipLaunchKernelGGL(k_line_eval<false>, dim3(n_lo), dim3(64), 0, h->stream, P, s, 0); }
        }
        if (pl.dp_max_nf > 0) { ScopedTimer t(h, "k_prior_m"); hipLaunchKernelGGL(k_prior_m, dim3((pl.dp_max_nf + 3) / 4, n_win), dim3(256), 0, h->stream, P, s); }
        if (n_pf && (use_lm || !with_imu)) { ScopedTimer t(h, "k_pf_cost"); hipLaunchKernelGGL(k_pf_eval<true>, dim3(n_pf), dim3(64), 0, h->stream, P, s); }
        if (use_lm) {
            ScopedTimer t(h, "k_lm_pass"); hipLaunchKernelGGL(pl.k_lm_pass, dim3(pl.lm_n_sub), dim3(LM_PASS_THREADS), pl.lds_pass, h->stream, P, s, mtk, pl.lm_sub_obs);
        }
        else
        { ScopedTimer t(h, "k_backsub"); hipLaunchKernelGGL(pl.k_backsub, dim3(n_tiles + (with_imu ? n_pf : 0)), dim3(BUILD_THREADS), pl.lds_back, h->stream, P, s, mtk); }
        if (pl.lg.n_long) { ScopedTimer t(h, "k_long_back"); hipLaunchKernelGGL(pl.k_long_back, dim3(pl.lg.n_long), dim3(LONG_THREADS), pl.lds_long_back, h->stream, P, pl.lg, s); }
        if (fork) (void)hipStreamWaitEvent(h->stream, h->ev_cost, 0);
        if (h->coll_fn) {
            { ScopedTimer t(h, "k_rank_partials"); hipLaunchKernelGGL(k_rank_partials, dim3(n_win), dim3(64), 0, h->stream, P, s, 1); }
            ScopedTimer t(h, "allreduce_step_partials");
            if (h->coll_fn(h->coll_ctx, P.rank_s, (int64_t)n_win * P.world * 4, (void*)h->stream) != 0) coll_ok = false;
        }
        if (P.decide_kernel) { ScopedTimer t(h, "k_decide"); hipLaunchKernelGGL(k_decide, dim3(n_win), dim3(pl.max_win_tiles > 4 * BUILD_THREADS ? 1024 : 64), 0, h->stream, P, s, 0); }
    }
    { ScopedTimer t(h, "k_final"); hipLaunchKernelGGL(k_decide, dim3(n_win), dim3(64), 0, h->stream, P, pl.slots - 1, 1); }
    return coll_ok;
}

// SADVIO_DEBUG & 4096: the in-kernel phase stamps of the solve that just finished
void print_debug_stamps(sadvio_ba_handle* h, int n_tiles) {
    long long ts[128];
    if (hipMemcpy(ts, h->d_dbg.p, sizeof(ts), hipMemcpyDeviceToHost) == hipSuccess) {
        fprintf(stderr, "[sadvio dbg] phase dt (us):");
        for (int i = 1; i < 16; i++) fprintf(stderr, " %d:%.2f", i, (ts[i] - ts[0]) * 0.01);
        fprintf(stderr, "  shader clock %.3f GHz\n[sadvio dbg] k_build:", (double)(ts[21] - ts[20]) / ((ts[15] - ts[0]) * 10.0));
        for (int i = 33; i < 43; i++) fprintf(stderr, " %d:%.2f", i, (ts[i] - ts[32]) * 0.01);
        fprintf(stderr, "\n[sadvio dbg] first IMU pair of k_build, us since its start (residual + Jacobian on lane 0 | decision | W J | entries + adds): %.2f %.2f %.2f %.2f, start %.2f us after tile 0",
                (ts[57] - ts[56]) * 0.01, (ts[58] - ts[56]) * 0.01, (ts[59] - ts[56]) * 0.01, (ts[60] - ts[56]) * 0.01, (ts[56] - ts[32]) * 0.01);
        fprintf(stderr, "\n[sadvio dbg] k_wchol_step (panel 1), us since the workgroup's start: look-ahead (operands in LDS | substituted | block updated | factored) %.2f %.2f %.2f %.2f",
                (ts[107] - ts[106]) * 0.01, (ts[108] - ts[106]) * 0.01, (ts[109] - ts[106]) * 0.01, (ts[110] - ts[106]) * 0.01);
        fprintf(stderr, " | tile workgroup 7, %.2f us after it (operands | substituted | end) %.2f %.2f %.2f | inverse workgroup, %.2f us after it: %.2f",
                (ts[114] - ts[106]) * 0.01, (ts[115] - ts[114]) * 0.01, (ts[116] - ts[114]) * 0.01, (ts[117] - ts[114]) * 0.01, (ts[120] - ts[106]) * 0.01, (ts[121] - ts[120]) * 0.01);
        fprintf(stderr, "\n[sadvio dbg] chol16 cycles since its first barrier (panel | trailing + next pivot, per block column):");
        for (int i = 65; i < 81; i++) fprintf(stderr, " %lld", ts[i] - ts[64]);
        fprintf(stderr, " | back-substitution %lld .. %lld | end %lld", ts[82] - ts[64], ts[83] - ts[64], ts[84] - ts[64]);
        fprintf(stderr, "\n[sadvio dbg] k_chol_panel / k_band_solve (fwd window 2: carry fresh chol store | fwd end | bwd window 2: load below steps | bwd end):");
        for (int i = 45; i < 55; i++) fprintf(stderr, " %d:%.2f", i - 44, (ts[i] - ts[44]) * 0.01);
        fprintf(stderr, "\n");
    }
#ifdef SADVIO_KERNEL_TS
    // every workgroup of one k_build launch: start / end relative to workgroup 0's start, and the CU it ran on
    std::vector<long long> wg(4 * (size_t)std::min(n_tiles, DBG_WG_MAX));
    if (!wg.empty() && hipMemcpy(wg.data(), h->d_dbg.p + DBG_WG_BASE, wg.size() * sizeof(long long), hipMemcpyDeviceToHost) == hipSuccess)
        for (size_t b = 0; b < wg.size() / 4; b++) {
            const unsigned hw = (unsigned)wg[4 * b + 2];
            fprintf(stderr, "[sadvio dbg] k_build wg %zu start %.2f end %.2f xcc %d se %u sh %u cu %u simd %u\n", b, (wg[4 * b] - wg[0]) * 0.01, (wg[4 * b + 1] - wg[0]) * 0.01,
                    (int)((wg[4 * b + 2] >> 32) & 15), (hw >> 13) & 7, (hw >> 12) & 1, (hw >> 8) & 15, (hw >> 4) & 3);
        }
    // the tile sums of that launch: how many waves are `uniform` (8 landmarks with the same key-frames in the same lanes), and the head lanes of each workgroup's fullest wave
    long long uni = 0, over32 = 0, hmax = 0, hsum = 0;
    for (size_t b = 0; b < wg.size() / 4; b++) {
        const long long heads = wg[4 * b + 3] & 0xffffffffLL;
        uni += wg[4 * b + 3] >> 32; hmax = std::max(hmax, heads); hsum += heads; over32 += heads > 32;
    }
    if (!wg.empty())
        fprintf(stderr, "[sadvio dbg] k_build tile sums: %lld uniform waves in %zu workgroups; most head lanes in a wave %lld (mean of the workgroups' fullest waves %.1f), workgroups with a wave above 32 heads %lld\n",
                uni, wg.size() / 4, hmax, (double)hsum / (double)(wg.size() / 4), over32);
#endif
}

// sadvio_ba_solve, step 1. The caller's options as the kernels take them; null: the defaults
int convert_options(sadvio_ba_handle* h, const sadvio_solve_options* opts, SolveOpts& o) {
    sadvio_solve_options defo;
    if (!opts) { sadvio_ba_default_options(&defo); opts = &defo; }
    if (opts->max_num_iterations < 0 || opts->max_num_iterations > 1000) { h->err = "solve: max_num_iterations out of range"; return SADVIO_E_INVALID_ARG; }
    memset(&o, 0, sizeof(o));   // it travels in DevPtrs, whose bytes are part of the graph key
    solve_opts_from(*opts, o);
    o.huber_a = opts->huber_a;
    // wall_clock64: 100 MHz. Not applied to a window sharded over several GPUs: the ranks' clocks would disagree on the slot
    o.max_time_ticks = (opts->max_solver_time_in_seconds > 0.0 && h->world == 1) ? opts->max_solver_time_in_seconds * 1e8 : 0.0;
    if (!(o.huber_a >= 0.0)) { h->err = "solve: huber_a must be >= 0"; return SADVIO_E_INVALID_ARG; }
    return SADVIO_OK;
}

// sadvio_ba_solve, step 3. Launch, as one graph where the handle asks for it
int launch_solve(sadvio_ba_handle* h, const SolvePlan& plan, const std::vector<BigPlan>& big) {
    bool coll_ok = true;
    if (h->cfg.use_graph && !h->cfg.profile_kernels && !h->coll_fn) {
        // the whole <= 20-iteration solve is one graph launch, re-captured whenever the plan differs from the captured one in any byte
        const unsigned char* pb = (const unsigned char*)&plan;
        const unsigned char* bb = (const unsigned char*)big.data();
        std::vector<unsigned char> key(pb, pb + sizeof(plan));
        key.insert(key.end(), bb, bb + big.size() * sizeof(BigPlan));
        if (!h->graph_exec || key != h->graph_key) {
            if (h->graph_exec) { (void)hipGraphExecDestroy(h->graph_exec); h->graph_exec = nullptr; }
            hipGraph_t g = nullptr;
            HIP_TRY(hipStreamBeginCapture(h->stream, hipStreamCaptureModeThreadLocal));
            enqueue_solve(h, plan, big);
            HIP_TRY(hipStreamEndCapture(h->stream, &g));
            HIP_TRY(hipGraphInstantiate(&h->graph_exec, g, nullptr, nullptr, 0));
            (void)hipGraphDestroy(g);
            h->graph_key.swap(key);
        }
        HIP_TRY(hipGraphLaunch(h->graph_exec, h->stream));
    } else {
        coll_ok = enqueue_solve(h, plan, big);
    }
    HIP_TRY(hipGetLastError());
    if (!coll_ok) { h->err = "solve: the all-reduce of the reduced system failed"; return SADVIO_E_RCCL; }
    return SADVIO_OK;
}

// sadvio_ba_solve, step 6. The final records as the handle's solved state and the caller's summaries (null: none asked for)
int solve_summaries(sadvio_ba_handle* h, const SolveOpts& o, const SolvePlan& plan, sadvio_solve_summary* summaries) {
    const int n_win = plan.P.n_win;
    h->fin.assign(h->h_final, h->h_final + n_win);
    h->deltas_cached = false;
    h->last_slots = plan.slots; h->last_one_round = plan.one_round;
    h->cov_huber_a = o.huber_a; h->cov_use_lm = plan.use_lm;
    h->cv.border_known.clear();   // (CovScratch: the border route's plans live from solve to solve)
    h->solved = true;
    int rc = SADVIO_OK;
    for (int w = 0; w < n_win; w++) {
        const LmState& s = h->fin[w].s;
        if (summaries) {
            sadvio_solve_summary& S = summaries[w];
            S.iterations = s.iter; S.num_successful_steps = s.n_success; S.num_unsuccessful_steps = s.n_unsuccess;
            S.termination = s.termination; S.initial_cost = s.initial_cost; S.final_cost = s.x_cost;
            S.fixed_cost = 0.5 * h->fin[w].fixed_cost; S.final_radius = s.radius;
        }
        if (s.termination == SADVIO_TERM_FAILURE) rc = SADVIO_E_NOT_USABLE;
    }
    return rc;
}

// sadvio_ba_get_deltas: window w's share of the solved deltas (any output may be null)
int read_deltas(sadvio_ba_handle* h, int32_t w, double* pose, double* lmk, double* dv, double* dba, double* dbg) {
    HIP_TRY(hipSetDevice(h->device));
    const WinDev& d = h->plan.wins[w].d;
    const int cur = h->fin[w].s.cur;
    // One read-back per solve: both buffers of every delta array go to a pinned host buffer with asynchronous copies and ONE
    // synchronisation (a pageable hipMemcpy per array and window costs 30 - 80 us each); every get_deltas of this solve is then
    // a host memcpy. Layout: xp [2][6 n_kf] | xl [2][3 n_lmk] | xv | xba | xbg [2][3 n_kf] each.
    const size_t nk = (size_t)h->plan.n_kf_tot, nl = (size_t)h->plan.n_lmk_tot;
    const size_t o_xp = 0, o_xl = o_xp + 12 * nk, o_xv = o_xl + 6 * nl, o_xba = o_xv + 6 * nk, o_xbg = o_xba + 6 * nk, total = o_xbg + 6 * nk;
    if (!h->deltas_cached) {
        if (h->h_deltas_cap < total) {
            if (h->h_deltas) (void)hipHostFree(h->h_deltas);
            h->h_deltas = nullptr; h->h_deltas_cap = 0;
            HIP_TRY(hipHostMalloc((void**)&h->h_deltas, sizeof(double) * (total + total / 2), hipHostMallocDefault));
            h->h_deltas_cap = total + total / 2;
        }
        bool any_imu = false;
        for (const auto& hw : h->plan.wins) any_imu |= hw.d.has_imu != 0;
        HIP_TRY(hipMemcpyAsync(h->h_deltas + o_xp, h->d_xp.p, sizeof(double) * 12 * nk, hipMemcpyDeviceToHost, h->stream));
        if (nl) HIP_TRY(hipMemcpyAsync(h->h_deltas + o_xl, h->d_xl.p, sizeof(double) * 6 * nl, hipMemcpyDeviceToHost, h->stream));
        if (any_imu) {
            HIP_TRY(hipMemcpyAsync(h->h_deltas + o_xv, h->d_xv.p, sizeof(double) * 6 * nk, hipMemcpyDeviceToHost, h->stream));
            HIP_TRY(hipMemcpyAsync(h->h_deltas + o_xba, h->d_xba.p, sizeof(double) * 6 * nk, hipMemcpyDeviceToHost, h->stream));
            HIP_TRY(hipMemcpyAsync(h->h_deltas + o_xbg, h->d_xbg.p, sizeof(double) * 6 * nk, hipMemcpyDeviceToHost, h->stream));
        } else {
            memset(h->h_deltas + o_xv, 0, sizeof(double) * 18 * nk);   // windows without IMU states: their deltas are never touched (zero)
        }
        HIP_TRY(hipStreamSynchronize(h->stream));
        h->deltas_cached = true;
    }
    if (pose) memcpy(pose, h->h_deltas + o_xp + (size_t)cur * 6 * nk + 6 * (size_t)d.kf_base, sizeof(double) * 6 * d.n_kf);
    if (lmk && d.n_lmk) memcpy(lmk, h->h_deltas + o_xl + (size_t)cur * 3 * nl + 3 * (size_t)d.lmk_base, sizeof(double) * 3 * d.n_lmk);
    double* outs[3] = {dv, dba, dbg};
    const size_t offs[3] = {o_xv, o_xba, o_xbg};
    for (int q = 0; q < 3; q++)
        if (outs[q]) memcpy(outs[q], h->h_deltas + offs[q] + (size_t)cur * 3 * nk + 3 * (size_t)d.kf_base, sizeof(double) * 3 * d.n_kf);
    return SADVIO_OK;
}

// sadvio_ba_get_line_deltas
int read_line_deltas(sadvio_ba_handle* h, int32_t w, double* line_delta6) {
    HIP_TRY(hipSetDevice(h->device));
    const WinDev& d = h->plan.wins[w].d;
    const int n = d.line_end - d.line_begin;
    if (n > 0) HIP_TRY(hipMemcpy(line_delta6, h->d_xline.p + (size_t)h->fin[w].s.cur * 6 * h->n_line_tot + 6 * (size_t)d.line_begin, sizeof(double) * 6 * n, hipMemcpyDeviceToHost));
    return SADVIO_OK;
}

// sadvio_ba_get_trace
int read_trace(sadvio_ba_handle* h, int32_t w, int32_t cap_rows, double* rows8, int32_t* n_rows) {
    HIP_TRY(hipSetDevice(h->device));
    const int stride = h->last_slots + 2;
    const int n = std::min(h->fin[w].s.iter + 1, stride);
    if (n_rows) *n_rows = n;
    const int m = std::min(n, cap_rows);
    if (m > 0) HIP_TRY(hipMemcpy(rows8, h->d_trace.p + (size_t)w * stride * 8, sizeof(double) * 8 * (size_t)m, hipMemcpyDeviceToHost));
    return SADVIO_OK;
}

}  // namespace
