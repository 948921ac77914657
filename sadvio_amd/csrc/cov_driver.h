// cov_driver.h — the host side of sadvio_ba_covariance as named steps
//   cov_check -> cov_routes -> cov_assemble -> cov_invert -> cov_landmarks -> cov_read_back
// Sigma_pp is formed densely (cov_invert) or, for a block-banded S, inside its band only (cov_invert_band, cov_band_kernels.h: the
// BAND route; cov_band_route says when) or, for a window that loop closures keep from being banded, inside the band of its core and
// on the rows of a small border (cov_invert_border, cov_border_kernels.h: the BORDER route; cov_border_route says when; its
// read-back is the band route's). On the band route k_cov_schur runs over the table of in-band key-frame pairs, no kernel
// reads an entry of Sigma outside the band, pair blocks outside the band come from band substitution, and the host receives the
// blocks asked for and nothing else.
// S and the landmark blocks have two assemblies: the plain one and the square-root one, which survives landmarks millimetres from a
// camera centre. cov_assemble serves both and branches on CovRoutes::sqrt where they differ; cov_steps says which runs
// (SADVIO_COV_SQRT) and holds the retry. cov_attempt and cov_steps take the last step as a callable: cov_read_back here, covx_cross
// in cov_cross_driver.h. What sadvio_ba_covariance_batch shares with this call on the host is here too: cov_check_request (the
// request's validation under the call's name), cov_wait, cov_not_usable, cov_pick_blocks and cov_pick_landmarks.
// A window with long tracks (handles created with SADVIO_CFG_LONG_TRACK_COVARIANCE; every other handle is refused in ba_capi.hip) adds
// cov_assemble_long to either assembly and k_cov_lmk_long to cov_landmarks (cov_long_kernels.h); without long tracks no launch changes.
// The kernels are cov_kernels.h's; the factorisation of S and the triangular inverse are marg_driver.h's (factor_unpivoted,
// prior_build_Z: the route sadvio_ba_sparsify takes to Sigma_k = Ak^-1), called as they are. Nothing of the solve is touched: the
// delta buffers, the final records, the trace and the handle's prior are read only; the work buffers are the handle's CovScratch
// and, inside the two borrowed routines, MargScratch.
// Part of the library's single translation unit (ba_capi.hip); not a public header.
#pragma once
#include <cassert>
#include <climits>
#include "ba_handle.h"
#include "cov_band_kernels.h"
#include "cov_border_kernels.h"
#include "cov_kernels.h"
#include "cov_kf_lists.h"
#include "cov_long_kernels.h"
#include "marg_driver.h"

namespace {

// Everything a call decides, behind cov_check: the steps read it.
struct CovRoutes {
    int cur = 0;            // delta buffer holding the final accepted state
    bool pix = true;        // pixel (else angular) visual factor
    int Np = 0;             // columns of the reduced system; 0: every key-frame constant, nothing kept — Sigma_ll = H_ll^-1
    bool kept = false;      // landmarks in the reduced system (k_cov_kept)
    bool dense = false;     // a dense prior is attached (k_cov_dense)
    bool want_lmk = false;  // landmark blocks asked for (k_cov_lmk)
    int G = 16;             // lanes per landmark of k_cov_lmk: 16 up to 8 free key-frames, else 64
    int n_lmk_out = 0;      // landmark blocks written
    bool band = false;      // the band route; then hb / bw / nb: block half-bandwidth, (hb + 1) * dpf, block column of the sweeps
    int hb = 0, bw = 0, nb = 0, dpf = 6;
    const CovBorderPlan* border = nullptr;   // the border route (then band is false): hb / bw are the core's hb' / bw'
    bool banded() const { return band || border != nullptr; }
    bool sqrt = false;      // the square-root assembly instead of the plain one (cov_assemble)
    int n_long = 0, long_first = 0, long_max_kf = 0;   // long tracks of the window, its first on the long list, LongArgs::max_kf (k_cov_long, k_cov_lmk_long)
};

// The band route's block column: 6 for dpf 6, 5 for dpf 15 (as k_band_solve)
inline int cov_band_nb(int dpf) { return dpf == 6 ? 6 : 5; }

// Does window w take the band route? Bandable: N_p > 0, bw < N_p (window_bandwidth: no dense prior, kept landmarks or lines) and the
// kernel's LDS image fits (bw + nb <= COVBAND_MAXW). SADVIO_COV_BAND unset: only a window the dense route refuses (N_p >= 2047);
// 1: every bandable window; 0: never.
bool cov_band_route(const sadvio_ba_handle* h, int w, int* hb_out = nullptr, int* bw_out = nullptr) {
    const WinDev& d = h->plan.wins[w].d;
    if (h->env.cov_band == 0 || d.Np <= 0) return false;
    int hb = 0;
    const int bw = window_bandwidth(h, w, &hb), nb = cov_band_nb(d.dpf);
    if (hb_out) *hb_out = hb;
    if (bw_out) *bw_out = bw;
    if (!(bw < d.Np && bw + nb <= COVBAND_MAXW && d.Np % nb == 0)) return false;
    return h->env.cov_band > 0 || d.Np + 1 > PCH_MAXN;
}

// The border route's plan of window w (cov_border_plan.h), made once per solve from the couplings window_bandwidth counts
const CovBorderPlan& cov_border_plan_of(sadvio_ba_handle* h, int w) {
    CovScratch& V = h->cv;
    const size_t n_win = h->plan.wins.size();
    if (V.border_known.size() != n_win) { V.border_known.assign(n_win, 0); V.border_plan.resize(n_win); }
    CovBorderPlan& P = V.border_plan[w];
    if (V.border_known[w]) return P;
    const WinDev& d = h->plan.wins[w].d;
    const LayoutPlan& L = h->plan;
    CovBorderCouplings Cp;
    Cp.n_free = d.n_free_kf;
    std::vector<int> f;
    for (int l = 0; l < d.n_lmk; l++) {   // (long tracks included: the observation lists hold every observation)
        f.clear();
        for (int o = L.lmk_ob[d.lmk_base + l]; o < L.lmk_oe[d.lmk_base + l]; o++) f.push_back(L.kf_fidx[L.obs_kf[o]]);
        Cp.add_landmark(f.data(), (int)f.size());
    }
    for (const ImuDev& q : h->imus_per_win[w]) Cp.add_pair(L.kf_fidx[q.kf_i], L.kf_fidx[q.kf_j]);
    if (w < (int)h->sparse_per_win.size())
        for (const sadvio_sparse_prior& sp : h->sparse_per_win[w])
            if (sp.type == SADVIO_SPARSE_RELATIVE_POSE) Cp.add_pair(L.kf_fidx[d.kf_base + sp.kf], L.kf_fidx[d.kf_base + sp.kf_b]);
    int hb_lim = cov_border_hb_max(d.dpf);
    if (h->env.cov_border_hb > 0) hb_lim = std::min(hb_lim, h->env.cov_border_hb);   // (tests; only ever lowers it)
    const bool fills = d.n_red > 0 || d.dp_n_full > 0 || d.line_end > d.line_begin || d.Np != d.n_free_kf * d.dpf;
    cov_border_plan(Cp, d.dpf, cov_band_nb(d.dpf), hb_lim, fills, P);
    V.border_known[w] = 1;
    return P;
}

// Does window w take the border route? Borderable (cov_border_plan.h) and, SADVIO_COV_BORDER unset: only a window that is refused
// otherwise (N_p >= 2047 and not on the band route); 1: every borderable window (a window without a closure edge is not borderable:
// it keeps the band route or the dense one); 0: never. The plan, or null.
const CovBorderPlan* cov_border_route(sadvio_ba_handle* h, int w) {
    const WinDev& d = h->plan.wins[w].d;
    if (h->env.cov_border == 0 || d.Np <= 0 || h->world > 1) return nullptr;
    if (h->env.cov_border < 0 && !(d.Np + 1 > PCH_MAXN && !cov_band_route(h, w))) return nullptr;
    const CovBorderPlan& P = cov_border_plan_of(h, w);
    return P.ok() ? &P : nullptr;
}

// An invalid argument of the call named `call` ("covariance" | "covariance_batch"): its text, its code
int cov_invalid(sadvio_ba_handle* h, const char* call, const char* what) {
    h->err = std::string(call) + what;
    return SADVIO_E_INVALID_ARG;
}

// 1. Request rq on window w, for sadvio_ba_covariance and for every item of sadvio_ba_covariance_batch: the window, then the
// request's counts, pointers and indices. through_lm: is a batch solved by the throughput kernels served (cov_batch_driver.h says why
// the batch call accepts one)? border_ok: does the caller serve the border route (sadvio_ba_covariance_cross does not)?
int cov_check_request(sadvio_ba_handle* h, const char* call, int w, const sadvio_cov_request* rq, bool through_lm, bool border_ok = true) {
    if (w < 0 || w >= (int)h->plan.wins.size()) return cov_invalid(h, call, ": window out of range");
    if (!rq) return cov_invalid(h, call, ": null request");
    const WinDev& d = h->plan.wins[w].d;
    if (d.line_end > d.line_begin) return cov_invalid(h, call, ": the window carries line landmarks");
    if (h->cov_use_lm && !through_lm) return cov_invalid(h, call, ": the batch was solved by the throughput kernels");
    if (rq->n_kf < 0 || rq->n_pair < 0 || rq->n_lmk < -1 || (rq->n_kf > 0 && !rq->kf) || (rq->n_pair > 0 && (!rq->pair_a || !rq->pair_b)) ||
        (rq->n_lmk > 0 && !rq->lmk)) return cov_invalid(h, call, ": request out of range");
    for (int i = 0; i < rq->n_kf; i++)
        if (rq->kf[i] < 0 || rq->kf[i] >= d.n_kf) return cov_invalid(h, call, ": key-frame index out of range");
    for (int i = 0; i < rq->n_pair; i++)
        if (rq->pair_a[i] < 0 || rq->pair_a[i] >= d.n_kf || rq->pair_b[i] < 0 || rq->pair_b[i] >= d.n_kf) return cov_invalid(h, call, ": key-frame index of a pair out of range");
    for (int i = 0; i < rq->n_lmk; i++)
        if (rq->lmk[i] < 0 || rq->lmk[i] >= d.n_lmk) return cov_invalid(h, call, ": landmark index out of range");
    if (d.Np + 1 > PCH_MAXN && !cov_band_route(h, w) && !(border_ok && cov_border_route(h, w))) return cov_invalid(h, call, ": the reduced system has 2047 columns or more");
    return SADVIO_OK;
}

// 1. State and arguments. Host work only.
int cov_check(sadvio_ba_handle* h, int w, const sadvio_cov_request* rq, bool border_ok = true) {
    if (h->world > 1) return cov_invalid(h, "covariance", ": the window is sharded over several GPUs (each rank holds a landmark partition only)");
    if (int rc = entry_state(h, "covariance", NOT_DEFERRED | NEED_SOLVED)) return rc;
    return cov_check_request(h, "covariance", w, rq, false, border_ok);
}

CovRoutes cov_routes(sadvio_ba_handle* h, int w, const sadvio_cov_request* rq, const double* lmk_cov, bool border_ok = true) {
    const WinDev& d = h->plan.wins[w].d;
    CovRoutes R;
    R.cur = h->fin[w].s.cur;
    R.pix = h->plan.factor_type == SADVIO_FACTOR_PIXEL;
    R.Np = d.Np;
    R.kept = d.kept_end > d.kept_begin;
    R.dense = d.dp_n_full > 0;
    R.n_lmk_out = rq->n_lmk < 0 ? d.n_lmk : rq->n_lmk;
    R.want_lmk = lmk_cov != nullptr && R.n_lmk_out > 0;
    R.G = d.n_free_kf <= 8 ? 16 : 64;
    R.band = cov_band_route(h, w, &R.hb, &R.bw);
    R.nb = cov_band_nb(d.dpf); R.dpf = d.dpf;
    R.border = border_ok ? cov_border_route(h, w) : nullptr;
    if (R.border) { R.band = false; R.hb = R.border->hb_core; R.bw = (R.hb + 1) * d.dpf; }
    R.long_first = h->plan.wins[w].long_begin; R.n_long = h->plan.wins[w].long_end - R.long_first; R.long_max_kf = h->plan.long_max_kf;
    return R;
}

CovDev cov_dev(sadvio_ba_handle* h, int w, const CovRoutes& R) {
    CovScratch& V = h->cv;
    CovDev C{};
    C.w = w; C.cur = R.cur; C.Np = R.Np; C.huber_a = h->cov_huber_a;
    C.ptab = V.ptab.p; C.hll = V.hll.p; C.hinv = V.hinv.p; C.status = V.status.p; C.ent_n = V.ent_n.p;
    C.ent_col = V.ent_col.p; C.ent_w = V.ent_w.p; C.ent_hpp = V.ent_hpp.p;
    C.S = V.S.p; C.Sig = V.Sig.p; C.lout = V.lout.p;
    C.pair_tab = R.banded() ? V.pair_tab.p : nullptr;
    C.is_long = R.n_long > 0 ? V.is_long.p : nullptr;
    return C;
}

// The long list as the covariance kernels take it (the solve plan's LongArgs, solve_driver.h)
LongArgs cov_long_args(const sadvio_ba_handle* h) {
    LongArgs A{};
    A.n_long = h->plan.n_long; A.max_kf = h->plan.long_max_kf;
    A.rec = h->d_long_rec.p; A.kf = h->d_long_kf.p; A.slot = h->d_long_slot.p;
    return A;
}

// On the band route every pair of free key-frames that observe one long track lies inside the band: window_bandwidth counts the
// track. On the border route every such pair lies inside the core's band or has a border member: the planner counts the track.
// (Asserted below unless NDEBUG is defined; k_cov_lmk_long reads Sigma_pp at those pairs only.)
[[maybe_unused]] bool cov_long_in_band(const sadvio_ba_handle* h, int w, const CovRoutes& R) {
    for (int i = R.long_first; i < R.long_first + R.n_long; i++) {
        const int* rec = &h->plan.long_rec[(size_t)LONG_REC * i];
        int lo = INT_MAX, hi = -1;
        for (int k = 0; k < rec[3]; k++) {
            int f = h->plan.kf_fidx[h->plan.long_kf[rec[2] + k]];
            if (f >= 0 && R.border) f = R.border->core_of[f];   // (-1: a border key-frame)
            if (f >= 0) { lo = std::min(lo, f); hi = std::max(hi, f); }
        }
        if (hi - lo > R.hb) return false;
    }
    return true;
}

// 2 (long tracks). The window's long tracks into the tables the tile assembly just filled for every other landmark: behind
// k_cov_tables and the tile assembly, in front of k_cov_schur(_sqrt). Q: the square-root assembly's tables (R.sqrt), else unused.
int cov_assemble_long(sadvio_ba_handle* h, const CovRoutes& R, const DevPtrs& P, const CovDev& C, const CovSqrtDev& Q) {
    if (R.n_long == 0) return SADVIO_OK;
    assert(!R.banded() || cov_long_in_band(h, C.w, R));
    HIP_TRY(hipMemsetAsync(C.is_long, 0, sizeof(int) * (size_t)h->plan.wins[C.w].d.n_lmk, h->stream));
    auto k = R.sqrt ? (R.pix ? k_cov_long<0, true> : k_cov_long<1, true>) : (R.pix ? k_cov_long<0, false> : k_cov_long<1, false>);
    ScopedTimer t(h, "k_cov_long");
    hipLaunchKernelGGL(k, dim3(R.n_long), dim3(LONG_THREADS), cov_long_lds_bytes(R.long_max_kf), h->stream, P, C, Q, cov_long_args(h), R.long_first);
    return SADVIO_OK;
}

// The band route's workgroups of k_cov_schur(_sqrt): the in-band pairs (a, b), a >= b, a - b <= hb, as a table on the device —
// nothing else of S can be non-zero. On the border route: the pairs inside the core's band (compacted index) and every pair with a
// border member. n_schur: how many.
int cov_pair_table(sadvio_ba_handle* h, const WinDev& d, const CovRoutes& R, int& n_schur) {
    CovScratch& V = h->cv;
    std::vector<int>& tab = V.h_pair_tab;
    tab.clear();
    if (R.border) {
        const std::vector<int>& core = R.border->core_of;
        for (int a = 0; a < d.n_free_kf; a++)
            for (int b = 0; b <= a; b++)
                if (core[a] < 0 || core[b] < 0 || core[a] - core[b] <= R.hb) { tab.push_back(a); tab.push_back(b); }
    } else {
        for (int a = 0; a < d.n_free_kf; a++)
            for (int b = std::max(0, a - R.hb); b <= a; b++) { tab.push_back(a); tab.push_back(b); }
    }
    n_schur = (int)tab.size() / 2;
    HIP_TRY(V.pair_tab.alloc(tab.size()));
    HIP_TRY(hipMemcpyAsync(V.pair_tab.p, tab.data(), sizeof(int) * tab.size(), hipMemcpyHostToDevice, h->stream));
    return SADVIO_OK;
}

// 2. Allocate; linearise at x*; S, full symmetric, in V.S. Two assemblies, which differ in the tile kernel, in the pair kernel and in
// what those keep per observation; everything else is one sequence.
//   plain (the class cov_assemble):             S = H_pp - sum_l H_pl H_ll^-1 H_lp
//   square-root (R.sqrt, cov_assemble_sqrt):    the same S in Gram form: per eliminated landmark J_l = Q1 R, C_a = Q1^T J_p,a, and block
//       (a, b) of S the sum over the landmark's rows of A_a^T A_b, A_a = [row is a's] J_p,a - Q1 C_a (cov_kernels.h) — never a difference
//       of two large matrices, so a landmark millimetres from a camera centre cannot turn S indefinite. The pair workgroups walk
//       key-frame -> landmark lists built here from the plan's observation lists and uploaded with the call.
int cov_assemble(sadvio_ba_handle* h, int w, const CovRoutes& R) {
    const WinDev& d = h->plan.wins[w].d;
    CovScratch& V = h->cv;
    const size_t nl = (size_t)std::max(d.n_lmk, 1), no = (size_t)std::max(d.n_obs, 1), nn = (size_t)std::max(R.Np, 1) * std::max(R.Np, 1);
    HIP_TRY(V.ptab.alloc((size_t)h->plan.n_kf_tot * POSE_TAB));
    HIP_TRY(V.hll.alloc(6 * nl)); HIP_TRY(V.hinv.alloc(6 * nl)); HIP_TRY(V.status.alloc(nl)); HIP_TRY(V.ent_n.alloc(nl)); HIP_TRY(V.lout.alloc(9 * nl));
    HIP_TRY(V.ent_col.alloc(no)); HIP_TRY(V.ent_w.alloc(COV_ENT_W * no));
    if (!R.sqrt) HIP_TRY(V.ent_hpp.alloc(COV_ENT_HPP * no));
    else { HIP_TRY(V.sq_jp.alloc(12 * no)); HIP_TRY(V.sq_q.alloc(6 * no)); HIP_TRY(V.sq_ent.alloc(no)); }
    HIP_TRY(V.S.alloc(nn)); HIP_TRY(V.Sig.alloc(nn));
    if (R.n_long > 0) HIP_TRY(V.is_long.alloc(nl));
    HIP_TRY(hipMemsetAsync(V.S.p, 0, sizeof(double) * nn, h->stream));
    SolveOpts so{};
    so.huber_a = h->cov_huber_a;
    const DevPtrs P = make_ptrs(h, so, h->last_slots + 2);
    int n_schur = d.n_free_kf * (d.n_free_kf + 1) / 2;
    if (R.banded() && R.Np > 0)
        if (int rc = cov_pair_table(h, d, R, n_schur)) return rc;
    CovSqrtDev Q{};
    if (R.sqrt) {
        cov_kf_lmk_lists(d.n_free_kf, d.n_lmk, h->plan.lmk_ob.data() + d.lmk_base, h->plan.lmk_oe.data() + d.lmk_base, h->plan.obs_kf.data(),
                         h->plan.kf_fidx.data(), V.h_kf_ptr, V.h_kf_lmk);
        HIP_TRY(V.kf_ptr.alloc(V.h_kf_ptr.size())); HIP_TRY(V.kf_lmk.alloc(V.h_kf_lmk.size()));
        HIP_TRY(hipMemcpyAsync(V.kf_ptr.p, V.h_kf_ptr.data(), sizeof(int) * V.h_kf_ptr.size(), hipMemcpyHostToDevice, h->stream));
        HIP_TRY(hipMemcpyAsync(V.kf_lmk.p, V.h_kf_lmk.data(), sizeof(int) * V.h_kf_lmk.size(), hipMemcpyHostToDevice, h->stream));
        Q = CovSqrtDev{V.sq_jp.p, V.sq_q.p, V.sq_ent.p, V.kf_ptr.p, V.kf_lmk.p};
    }
    const CovDev C = cov_dev(h, w, R);
    ScopedTimer t(h, R.sqrt ? "cov_assemble_sqrt" : "cov_assemble");
    const int n_tab = std::max(d.n_kf, d.n_lmk);
    hipLaunchKernelGGL(k_cov_tables, dim3((n_tab + 255) / 256), dim3(256), 0, h->stream, P, C, V.ptab.p);
    const int n_tiles = d.tile_end - d.tile_begin;
    if (n_tiles > 0) {
        if (R.sqrt) hipLaunchKernelGGL(R.pix ? k_cov_assemble_sqrt<0> : k_cov_assemble_sqrt<1>, dim3(n_tiles), dim3(COV_THREADS), 0, h->stream, P, C, Q);
        else hipLaunchKernelGGL(R.pix ? k_cov_assemble<0> : k_cov_assemble<1>, dim3(n_tiles), dim3(COV_THREADS), 0, h->stream, P, C);
    }
    if (int rc = cov_assemble_long(h, R, P, C, Q)) return rc;
    if (R.Np == 0) { HIP_TRY(hipGetLastError()); return SADVIO_OK; }
    if (d.n_free_kf > 0) {   // (band route, long tracks: a class of its own inside the assembly's span, for the profile)
        ScopedTimer ts(h, R.banded() || R.n_long > 0 ? (R.sqrt ? "k_cov_schur_sqrt" : "k_cov_schur") : nullptr);
        if (R.sqrt) hipLaunchKernelGGL(k_cov_schur_sqrt, dim3(n_schur), dim3(COV_SCHUR_THREADS), 0, h->stream, P, C, Q);
        else hipLaunchKernelGGL(k_cov_schur, dim3(n_schur), dim3(COV_SCHUR_THREADS), 0, h->stream, P, C);
    }
    if (R.kept) hipLaunchKernelGGL(R.pix ? k_cov_kept<0> : k_cov_kept<1>, dim3(1), dim3(64), 0, h->stream, P, C);
    {
        ScopedTimer tf(h, R.banded() ? "k_cov_factors" : nullptr);
        hipLaunchKernelGGL(k_cov_factors, dim3(1), dim3(64), 0, h->stream, P, C);
    }
    if (R.dense) hipLaunchKernelGGL(k_cov_dense, dim3((unsigned)(((long long)d.dp_n * d.dp_n + 255) / 256)), dim3(256), 0, h->stream, P, C);
    HIP_TRY(hipGetLastError());
    return SADVIO_OK;
}

// 3. Sigma_pp = S^-1: unpivoted Cholesky with every pivot tested, triangular inverse Z = G^-T, Sigma_pp = Z^T Z.
// usable = false: a pivot is not safely positive (gauge not fixed).
CovBand cov_band_dev(sadvio_ba_handle* h, const CovRoutes& R) {
    CovScratch& V = h->cv;
    CovBand B{};
    B.n = R.Np; B.bw = R.bw; B.M = R.bw + R.nb; B.dpf = R.dpf;
    B.tau = -pchol_tau(R.Np, SADVIO_EIG_CUT_REFERENCE);          // the reference's cut is an absolute pivot floor (a negative tau_rel)
    B.safe_rel = 1024.0 * R.Np * 2.220446049250313e-16;          // run_wfac's
    B.S = V.S.p; B.Sig = V.Sig.p; B.Lb = V.Lb.p; B.Linv = V.Linv.p; B.flag = V.bflag.p;
    return B;
}

// 3 (band route). The band of Sigma_pp: band Cholesky with every pivot tested, then the Takahashi recursion. Two launches whatever
// N_p; no host wait: a failed pivot sets V.bflag, which cov_read_back_band reads behind the call's one wait.
int cov_invert_band(sadvio_ba_handle* h, const CovRoutes& R) {
    CovScratch& V = h->cv;
    const int M = R.bw + R.nb;
    HIP_TRY(V.Lb.alloc((size_t)R.Np * M)); HIP_TRY(V.Linv.alloc((size_t)R.Np * R.nb)); HIP_TRY(V.bflag.alloc(2));
    HIP_TRY(hipMemsetAsync(V.bflag.p, 0, sizeof(int) * 2, h->stream));
    const CovBand B = cov_band_dev(h, R);
    const size_t lds = covband_lds_bytes(M, R.nb);
    auto kc = R.nb == 6 ? k_cov_band_chol<6> : k_cov_band_chol<5>;
    auto ks = R.nb == 6 ? k_cov_band_sel<6> : k_cov_band_sel<5>;
    HIP_TRY(hipFuncSetAttribute((const void*)kc, hipFuncAttributeMaxDynamicSharedMemorySize, (int)covband_lds_bytes(COVBAND_MAXW, R.nb)));
    HIP_TRY(hipFuncSetAttribute((const void*)ks, hipFuncAttributeMaxDynamicSharedMemorySize, (int)covband_lds_bytes(COVBAND_MAXW, R.nb)));
    { ScopedTimer t(h, "cov_band"); hipLaunchKernelGGL(kc, dim3(1), dim3(COVBAND_THREADS), lds, h->stream, B); }
    { ScopedTimer t(h, "cov_band_sel"); hipLaunchKernelGGL(ks, dim3(1), dim3(COVBAND_THREADS), lds, h->stream, B); }
    HIP_TRY(hipGetLastError());
    return SADVIO_OK;
}

// The border route's two views of its buffers: the core as the band kernels take it (compacted: n = n_b, S and Sigma the compacted
// images), and the whole of it as cov_border_kernels.h's take it. The pivot tests keep S's figures (tau and safe_rel of N_p).
CovBand cov_border_band_dev(sadvio_ba_handle* h, const CovRoutes& R) {
    CovScratch& V = h->cv;
    CovBand B = cov_band_dev(h, R);
    B.n = R.border->n_core() * R.dpf;
    B.S = V.bSb.p; B.Sig = V.bSigc.p;
    return B;
}
CovBorder cov_border_dev(sadvio_ba_handle* h, const CovRoutes& R) {
    CovScratch& V = h->cv;
    const CovBand Bc = cov_border_band_dev(h, R);
    CovBorder B{};
    B.n = R.Np; B.nc = Bc.n; B.m = R.Np - Bc.n; B.bw = Bc.bw; B.M = Bc.M; B.dpf = R.dpf; B.tau = Bc.tau; B.safe_rel = Bc.safe_rel;
    B.perm = V.bperm.p; B.S = V.S.p; B.Sig = V.Sig.p; B.Sb = V.bSb.p; B.Sigc = V.bSigc.p; B.Lb = V.Lb.p;
    B.Ct = V.bCt.p; B.Dm = V.bDm.p; B.W = V.bW.p; B.Z = V.bZ.p; B.Tinv = V.bTinv.p; B.flag = V.bflag.p;
    return B;
}

// 3 (border route). Split S into [B C; C^T D] by the plan; the band route's two sweeps on B; W = B^-1 C; the Schur complement T on
// the border, factored with every pivot tested; the corrections into Sigma at its natural positions. Six launches whatever N_p; no
// host wait: a failed pivot of B or of T sets V.bflag, which cov_read_back_band reads behind the call's one wait.
int cov_invert_border(sadvio_ba_handle* h, const CovRoutes& R) {
    CovScratch& V = h->cv;
    const CovBorderPlan& P = *R.border;
    const int dpf = R.dpf, nc = P.n_core() * dpf, m = (int)P.border.size() * dpf, M = R.bw + R.nb;
    HIP_TRY(V.Lb.alloc((size_t)nc * M)); HIP_TRY(V.Linv.alloc((size_t)nc * R.nb)); HIP_TRY(V.bflag.alloc(2));
    HIP_TRY(V.bSb.alloc((size_t)nc * nc)); HIP_TRY(V.bSigc.alloc((size_t)nc * nc)); HIP_TRY(V.bCt.alloc((size_t)m * nc)); HIP_TRY(V.bDm.alloc((size_t)m * m));
    HIP_TRY(V.bW.alloc((size_t)m * nc)); HIP_TRY(V.bZ.alloc((size_t)m * nc)); HIP_TRY(V.bTinv.alloc((size_t)m * m)); HIP_TRY(V.bperm.alloc((size_t)R.Np));
    V.h_bperm.resize((size_t)R.Np);
    for (size_t p = 0; p < P.order.size(); p++)
        for (int q = 0; q < dpf; q++) V.h_bperm[p * dpf + q] = P.order[p] * dpf + q;
    HIP_TRY(hipMemcpyAsync(V.bperm.p, V.h_bperm.data(), sizeof(int) * (size_t)R.Np, hipMemcpyHostToDevice, h->stream));
    HIP_TRY(hipMemsetAsync(V.bflag.p, 0, sizeof(int) * 2, h->stream));
    const CovBand Bc = cov_border_band_dev(h, R);
    const CovBorder B = cov_border_dev(h, R);
    const size_t lds = covband_lds_bytes(M, R.nb);
    auto kc = R.nb == 6 ? k_cov_band_chol<6> : k_cov_band_chol<5>;
    auto ks = R.nb == 6 ? k_cov_band_sel<6> : k_cov_band_sel<5>;
    HIP_TRY(hipFuncSetAttribute((const void*)kc, hipFuncAttributeMaxDynamicSharedMemorySize, (int)covband_lds_bytes(COVBAND_MAXW, R.nb)));
    HIP_TRY(hipFuncSetAttribute((const void*)ks, hipFuncAttributeMaxDynamicSharedMemorySize, (int)covband_lds_bytes(COVBAND_MAXW, R.nb)));
    HIP_TRY(hipFuncSetAttribute((const void*)k_cov_border_schur, hipFuncAttributeMaxDynamicSharedMemorySize, (int)covborder_lds_bytes(COV_BORDER_MAXM)));
    {
        const long long total = (long long)nc * R.bw + (long long)m * nc + (long long)m * m;
        ScopedTimer t(h, "cov_border_split");
        hipLaunchKernelGGL(k_cov_border_split, dim3((unsigned)((total + COVBAND_THREADS - 1) / COVBAND_THREADS)), dim3(COVBAND_THREADS), 0, h->stream, B);
    }
    { ScopedTimer t(h, "cov_band"); hipLaunchKernelGGL(kc, dim3(1), dim3(COVBAND_THREADS), lds, h->stream, Bc); }
    { ScopedTimer t(h, "cov_band_sel"); hipLaunchKernelGGL(ks, dim3(1), dim3(COVBAND_THREADS), lds, h->stream, Bc); }
    { ScopedTimer t(h, "cov_border_solve"); hipLaunchKernelGGL(k_cov_border_solve, dim3((unsigned)P.border.size()), dim3(COVBAND_THREADS), 0, h->stream, B); }
    { ScopedTimer t(h, "cov_border_schur"); hipLaunchKernelGGL(k_cov_border_schur, dim3(1), dim3(COVBAND_THREADS), covborder_lds_bytes(m), h->stream, B); }
    { ScopedTimer t(h, "cov_border_apply"); hipLaunchKernelGGL(k_cov_border_apply, dim3((unsigned)P.n_core() + 1), dim3(COVBAND_THREADS), 0, h->stream, B, R.hb); }
    HIP_TRY(hipGetLastError());
    return SADVIO_OK;
}

int cov_invert(sadvio_ba_handle* h, const CovRoutes& R, bool& usable) {
    usable = true;
    if (R.Np == 0) return SADVIO_OK;
    if (R.border) return cov_invert_border(h, R);
    if (R.band) return cov_invert_band(h, R);
    CovScratch& V = h->cv;
    MargScratch& M = h->mg;
    const int n = R.Np;
    const size_t nn = (size_t)n * n;
    HIP_TRY(V.V.alloc(nn)); HIP_TRY(V.Lx.alloc(nn)); HIP_TRY(V.G.alloc(nn)); HIP_TRY(V.Z.alloc(nn));
    HIP_TRY(M.wtmp.alloc((size_t)n + 16)); HIP_TRY(M.flag.alloc(8));
    ScopedTimer t(h, "cov_invert");   // (spans the one host wait of the pivot test)
    HIP_TRY(hipMemcpyAsync(V.V.p, V.S.p, sizeof(double) * nn, hipMemcpyDeviceToDevice, h->stream));
    HIP_TRY(hipMemsetAsync(M.wtmp.p, 0, sizeof(double) * ((size_t)n + 16), h->stream));
    bool ok = false;
    if (int rc = factor_unpivoted(h, V.V.p, n, M.wtmp.p + 8, V.Lx.p, V.S.p, (long long)n, pchol_tau(n, SADVIO_EIG_CUT_REFERENCE), V.G.p, V.step_of, ok)) {
        if (rc == SADVIO_E_HIP) h->err = "covariance: HIP error in the unpivoted Cholesky";
        return rc;
    }
    if (!ok) { usable = false; return SADVIO_OK; }
    if (int rc = prior_build_Z(h, V.G.p, n, n, SADVIO_PRIOR_FORM_CHOLESKY, V.step_of.p, V.Z.p, SADVIO_EIG_CUT_REFERENCE)) return rc;
    launch_mgemm(h, V.Sig.p, n, V.Z.p, 1LL, (long long)n, V.Z.p, (long long)n, 1LL, n, n, n, 1.0, 0.0);
    HIP_TRY(hipGetLastError());
    return SADVIO_OK;
}

// 4. Sigma_ll of every landmark of the window
int cov_landmarks(sadvio_ba_handle* h, int w, const CovRoutes& R) {
    const WinDev& d = h->plan.wins[w].d;
    if (!R.want_lmk || d.n_lmk == 0) return SADVIO_OK;
    SolveOpts so{};
    const DevPtrs P = make_ptrs(h, so, h->last_slots + 2);
    const CovDev C = cov_dev(h, w, R);
    const int per = COV_THREADS / R.G;
    if (R.n_long > 0) {   // the long tracks' blocks: k_cov_lmk below skips them (CovDev::is_long)
        ScopedTimer tl(h, "k_cov_lmk_long");
        hipLaunchKernelGGL(R.sqrt ? k_cov_lmk_long<true> : k_cov_lmk_long<false>, dim3(R.n_long), dim3(LONG_THREADS), 0, h->stream, P, C, cov_long_args(h), R.long_first);
    }
    ScopedTimer t(h, "k_cov_lmk");
    if (R.sqrt) hipLaunchKernelGGL((R.G == 16 ? k_cov_lmk<16, true> : k_cov_lmk<64, true>), dim3((d.n_lmk + per - 1) / per), dim3(COV_THREADS), 0, h->stream, P, C);
    else hipLaunchKernelGGL(R.G == 16 ? k_cov_lmk<16> : k_cov_lmk<64>, dim3((d.n_lmk + per - 1) / per), dim3(COV_THREADS), 0, h->stream, P, C);
    HIP_TRY(hipGetLastError());
    return SADVIO_OK;
}

// The call's wait, and the kernel timers behind it
int cov_wait(sadvio_ba_handle* h) {
    HIP_TRY(hipStreamSynchronize(h->stream));
    if (h->cfg.profile_kernels) collect_timers(h);
    return SADVIO_OK;
}

// The refusal of a window whose S failed a pivot test, behind the call's wait (waited: the caller has waited already)
const char* const COV_NOT_USABLE = "covariance: the reduced information matrix is not positive definite (gauge not fixed: no constant key-frame, no prior)";
int cov_not_usable(sadvio_ba_handle* h, bool waited = false) {
    if (!waited)
        if (int rc = cov_wait(h)) return rc;
    h->err = COV_NOT_USABLE;
    return SADVIO_E_NOT_USABLE;
}

// The key-frame and pair blocks asked for (null: not wanted), dpf x dpf each, out of Sigma_pp = sig [n][n] by free index; zero where
// a key-frame is constant
void cov_pick_blocks(const LayoutPlan& plan, const WinDev& d, const sadvio_cov_request* rq, const double* sig, int n, double* kf_cov, double* pair_cov) {
    const int dpf = d.dpf;
    auto block = [&](int ka, int kb, double* out) {
        const int fa = plan.kf_fidx[d.kf_base + ka], fb = plan.kf_fidx[d.kf_base + kb];
        for (int i = 0; i < dpf; i++)
            for (int j = 0; j < dpf; j++) out[i * dpf + j] = (fa >= 0 && fb >= 0 && n > 0) ? sig[(size_t)(fa * dpf + i) * n + fb * dpf + j] : 0.0;
    };
    if (kf_cov) for (int i = 0; i < rq->n_kf; i++) block(rq->kf[i], rq->kf[i], kf_cov + (size_t)i * dpf * dpf);
    if (pair_cov) for (int i = 0; i < rq->n_pair; i++) block(rq->pair_a[i], rq->pair_b[i], pair_cov + (size_t)i * dpf * dpf);
}

// The landmark blocks asked for out of the window's table lout [n_lmk][9], and how many of the landmarks asked for are singular by
// status [n_lmk] (either output null: not wanted, and its table is not read)
void cov_pick_landmarks(const sadvio_cov_request* rq, const WinDev& d, const double* lout, const int* status, double* lmk_cov, int32_t* n_lmk_singular) {
    const int n_out = rq->n_lmk < 0 ? d.n_lmk : rq->n_lmk;
    if (lmk_cov && rq->n_lmk < 0 && n_out > 0) memcpy(lmk_cov, lout, 72 * (size_t)n_out);
    int n_sing = 0;
    for (int i = 0; i < n_out; i++) {
        const int l = rq->n_lmk < 0 ? i : rq->lmk[i];
        if (lmk_cov && rq->n_lmk >= 0) memcpy(lmk_cov + 9 * (size_t)i, lout + 9 * (size_t)l, 72);
        if (n_lmk_singular) n_sing += status[l] == COV_LMK_SINGULAR ? 1 : 0;
    }
    if (n_lmk_singular) *n_lmk_singular = n_sing;
}

// 5 (band route, border route). The columns of the pair blocks outside the band by substitution with L's band, one workgroup per distinct column
// key-frame: the canonical block is (a, b), a > b in free index, and (b, a) is read as its transpose, so pair(a, b) and
// pair(b, a)^T agree to the bit and a pair's bits do not depend on what else was asked for. The blocks asked for are gathered on the
// device; one wait; SADVIO_E_NOT_USABLE with the outputs untouched when a pivot failed its test. On the border route a block with a
// border key-frame is read where k_cov_border_apply wrote it, the band is the core's in compacted index, and a block of two core
// key-frames outside it is the column of B^-1 plus the Z W^T term (k_cov_border_gather).
int cov_read_back_band(sadvio_ba_handle* h, int w, const sadvio_cov_request* rq, const CovRoutes& R, double* kf_cov, double* pair_cov, double* lmk_cov,
                       int32_t* n_lmk_singular) {
    const WinDev& d = h->plan.wins[w].d;
    CovScratch& V = h->cv;
    const int n = R.Np, dpf = d.dpf, bs = dpf * dpf;
    const int nk = kf_cov ? rq->n_kf : 0, np = pair_cov ? rq->n_pair : 0, nblk = nk + np;
    std::vector<int>& tab = V.h_gtab; std::vector<int>& xcol = V.h_xcol;
    tab.assign(4 * (size_t)std::max(nblk, 1), 0); xcol.clear();
    std::vector<int> x_of(d.n_free_kf, -1);
    for (int e = 0; e < nblk; e++) {
        const int ka = e < nk ? rq->kf[e] : rq->pair_a[e - nk], kb = e < nk ? ka : rq->pair_b[e - nk];
        const int fa = h->plan.kf_fidx[d.kf_base + ka], fb = h->plan.kf_fidx[d.kf_base + kb];
        int* T = &tab[4 * (size_t)e];
        if (fa < 0 || fb < 0) { T[0] = COVBAND_G_ZERO; continue; }
        const int ca = R.border ? R.border->core_of[fa] : fa, cb = R.border ? R.border->core_of[fb] : fb;   // index in the band (-1: a border key-frame)
        if (ca < 0 || cb < 0 || std::abs(ca - cb) <= R.hb) { T[0] = COVBAND_G_SIG; T[1] = fa * dpf; T[2] = fb * dpf; continue; }
        const int lo = std::min(ca, cb), hi = std::max(ca, cb);
        if (x_of[lo] < 0) { x_of[lo] = (int)xcol.size(); xcol.push_back(lo * dpf); }
        T[0] = ca > cb ? COVBAND_G_COL : COVBAND_G_COLT; T[1] = hi * dpf; T[2] = lo * dpf; T[3] = x_of[lo];
    }
    const CovBand B = R.border ? cov_border_band_dev(h, R) : cov_band_dev(h, R);
    std::vector<double>& out = V.h_sig; std::vector<double>& lo = V.h_lout;
    if (nblk > 0) {
        HIP_TRY(V.gtab.alloc(tab.size())); HIP_TRY(V.gout.alloc((size_t)nblk * bs));
        HIP_TRY(hipMemcpyAsync(V.gtab.p, tab.data(), sizeof(int) * tab.size(), hipMemcpyHostToDevice, h->stream));
        if (!xcol.empty()) {
            HIP_TRY(V.xcol.alloc(xcol.size())); HIP_TRY(V.X.alloc(xcol.size() * (size_t)dpf * B.n));
            HIP_TRY(hipMemcpyAsync(V.xcol.p, xcol.data(), sizeof(int) * xcol.size(), hipMemcpyHostToDevice, h->stream));
            ScopedTimer t(h, "cov_band_pairs");
            hipLaunchKernelGGL(k_cov_band_cols, dim3((unsigned)xcol.size()), dim3(COVBAND_THREADS), 0, h->stream, B, (const int*)V.xcol.p, V.X.p);
        }
        {
            ScopedTimer t(h, "cov_band_gather");
            if (R.border) hipLaunchKernelGGL(k_cov_border_gather, dim3(nblk), dim3(COVBAND_THREADS), 0, h->stream, cov_border_dev(h, R), (const int*)V.gtab.p, (const double*)V.X.p, V.gout.p);
            else hipLaunchKernelGGL(k_cov_band_gather, dim3(nblk), dim3(COVBAND_THREADS), 0, h->stream, B, (const int*)V.gtab.p, (const double*)V.X.p, V.gout.p);
        }
        HIP_TRY(hipGetLastError());
        out.resize((size_t)nblk * bs);
        HIP_TRY(hipMemcpyAsync(out.data(), V.gout.p, sizeof(double) * (size_t)nblk * bs, hipMemcpyDeviceToHost, h->stream));
    }
    if (R.want_lmk) {
        lo.resize(9 * (size_t)d.n_lmk);
        HIP_TRY(hipMemcpyAsync(lo.data(), V.lout.p, sizeof(double) * 9 * (size_t)d.n_lmk, hipMemcpyDeviceToHost, h->stream));
    }
    std::vector<int> st;
    if (n_lmk_singular && d.n_lmk > 0) {
        st.resize(d.n_lmk);
        HIP_TRY(hipMemcpyAsync(st.data(), V.status.p, sizeof(int) * (size_t)d.n_lmk, hipMemcpyDeviceToHost, h->stream));
    }
    int flag[2] = {0, 0};
    HIP_TRY(hipMemcpyAsync(flag, V.bflag.p, sizeof(flag), hipMemcpyDeviceToHost, h->stream));
    if (int rc = cov_wait(h)) return rc;
    if (flag[0] != 0) return cov_not_usable(h, true);
    if (nk > 0) memcpy(kf_cov, out.data(), sizeof(double) * (size_t)nk * bs);
    if (np > 0) memcpy(pair_cov, out.data() + (size_t)nk * bs, sizeof(double) * (size_t)np * bs);
    cov_pick_landmarks(rq, d, lo.data(), st.data(), lmk_cov, n_lmk_singular);
    return SADVIO_OK;
}

// 5. One wait; the caller's blocks are picked from Sigma_pp and the landmark table on the host
int cov_read_back(sadvio_ba_handle* h, int w, const sadvio_cov_request* rq, const CovRoutes& R, double* kf_cov, double* pair_cov, double* lmk_cov,
                  int32_t* n_lmk_singular) {
    const WinDev& d = h->plan.wins[w].d;
    CovScratch& V = h->cv;
    const int n = R.Np, dpf = d.dpf;
    if (R.banded()) return cov_read_back_band(h, w, rq, R, kf_cov, pair_cov, lmk_cov, n_lmk_singular);
    std::vector<double>& sig = V.h_sig; std::vector<double>& lo = V.h_lout;
    const bool want_pp = n > 0 && ((kf_cov && rq->n_kf > 0) || (pair_cov && rq->n_pair > 0));
    if (want_pp) { sig.resize((size_t)n * n); HIP_TRY(hipMemcpyAsync(sig.data(), V.Sig.p, sizeof(double) * (size_t)n * n, hipMemcpyDeviceToHost, h->stream)); }
    if (R.want_lmk) {
        lo.resize(9 * (size_t)d.n_lmk);
        HIP_TRY(hipMemcpyAsync(lo.data(), V.lout.p, sizeof(double) * 9 * (size_t)d.n_lmk, hipMemcpyDeviceToHost, h->stream));
    }
    std::vector<int> st;
    if (n_lmk_singular && d.n_lmk > 0) {
        st.resize(d.n_lmk);
        HIP_TRY(hipMemcpyAsync(st.data(), V.status.p, sizeof(int) * (size_t)d.n_lmk, hipMemcpyDeviceToHost, h->stream));
    }
    if (int rc = cov_wait(h)) return rc;
    cov_pick_blocks(h->plan, d, rq, sig.data(), n, kf_cov, pair_cov);
    cov_pick_landmarks(rq, d, lo.data(), st.data(), lmk_cov, n_lmk_singular);
    return SADVIO_OK;
}

// Steps 2 to 5 with the assembly R names; last(R) is step 5, the call's wait and its outputs (cov_read_back for sadvio_ba_covariance,
// covx_cross for sadvio_ba_covariance_cross). SADVIO_E_NOT_USABLE: a pivot of S failed its test; the outputs are untouched.
template <class Last>
int cov_attempt(sadvio_ba_handle* h, int w, const CovRoutes& R, const Last& last) {
    if (int rc = cov_assemble(h, w, R)) return rc;
    bool usable = true;
    if (int rc = cov_invert(h, R, usable)) return rc;
    if (!usable) return cov_not_usable(h);
    if (int rc = cov_landmarks(h, w, R)) return rc;
    return last(R);
}

// The assembly of a call (SADVIO_COV_SQRT, read once in EnvCfg). Unset: the plain one, and only when the pivot tests refuse its S
// (behind the call's wait on either route) the square-root one, with a second inversion, a second test and one further wait; a window
// the plain form serves keeps its bits, a refused one pays one more assembly before the same refusal. 1: square-root from the
// start. 0: plain only.
template <class Last>
int cov_steps(sadvio_ba_handle* h, int w, CovRoutes R, const Last& last) {
    R.sqrt = h->env.cov_sqrt == 1;
    int rc = cov_attempt(h, w, R, last);
    if (rc == SADVIO_E_NOT_USABLE && !R.sqrt && h->env.cov_sqrt != 0) {
        R.sqrt = true;
        rc = cov_attempt(h, w, R, last);
    }
    return rc;
}

// cov_read_back as the last step of cov_attempt / cov_steps
auto cov_read_back_into(sadvio_ba_handle* h, int w, const sadvio_cov_request* rq, double* kf_cov, double* pair_cov, double* lmk_cov, int32_t* n_lmk_singular) {
    return [=](const CovRoutes& R) { return cov_read_back(h, w, rq, R, kf_cov, pair_cov, lmk_cov, n_lmk_singular); };
}

int cov_run(sadvio_ba_handle* h, int w, const sadvio_cov_request* rq, double* kf_cov, double* pair_cov, double* lmk_cov, int32_t* n_lmk_singular) {
    if (int rc = cov_check(h, w, rq)) return rc;
    HIP_TRY(hipSetDevice(h->device));
    return cov_steps(h, w, cov_routes(h, w, rq, lmk_cov), cov_read_back_into(h, w, rq, kf_cov, pair_cov, lmk_cov, n_lmk_singular));
}

}  // namespace
