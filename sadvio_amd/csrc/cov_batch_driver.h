// cov_batch_driver.h — the host side of sadvio_ba_covariance_batch as named steps
//   covb_check -> covb_routes -> covb_groups -> covb_assemble -> covb_invert -> covb_landmarks -> covb_read_back
// Item i is what sadvio_ba_covariance(h, items[i].w, &items[i].rq, ..) defines. The device works per UNIT, a window named by at least
// one item: the items of a window share its assembly, its Sigma_pp and its landmark table, and differ only in the blocks the host
// picks for them. Units whose N_p is at most COVB_CAP (route LDS) or zero (route NONE) are processed in groups whose work arrays
// stay under the scratch budget; a group is one launch sequence on the handle's stream (cov_batch_kernels.h), its results go to
// pinned host memory with one asynchronous copy, and the call waits once, after the last group. A unit above the cap (route DENSE)
// goes item by item through cov_driver.h's steps (cov_steps), with the wait that route has; so does a unit on the band route (route
// BAND, cov_driver.h: cov_band_route), whatever its N_p. What the two calls share on the host is cov_driver.h's and is called from
// here: cov_check_request (an item's request, under this call's name), cov_wait, cov_pick_blocks and cov_pick_landmarks.
// The square-root assembly (cov_driver.h: cov_steps, SADVIO_COV_SQRT) exists on the single call's steps only. DENSE and BAND items
// inherit its choice and its retry. With the variable = 1 the LDS items go down the DENSE route and the NONE items through the same
// steps; with it unset, an LDS item whose unit failed the pivot test is retried on its own through those steps in square-root form
// behind the call's wait (covb_retry_item), and items that were served keep their bits.
// Long tracks (ba_capi.hip refuses them unless the handle has SADVIO_CFG_LONG_TRACK_COVARIANCE | SADVIO_CFG_LONG_TRACK_BATCH): a group
// whose units hold some uploads a work table behind its unit table (covb_long_plan.h: unit | index on the long list, units and tracks
// ascending) and launches k_covb_long behind k_covb_assemble and k_covb_lmk_long behind k_covb_lmk, one workgroup per row; such a unit
// gets a zeroed is_long array from the int pool. A group without long tracks takes the launches it always took. Items on the single
// call's steps are served by cov_driver.h's long kernels.
//
// After a solve by the throughput kernels (lm_kernels.h). sadvio_ba_covariance refuses such a batch; this call accepts it, on these
// grounds. (i) Both solve paths keep two delta buffers per array and LmState::cur names the one holding the accepted state x: k_solve
// (shared by both paths) writes the candidate poses to xp[1 - cur]; k_lm_pass reads xl[cur] and writes the candidate landmarks to
// xl[1 - cur] exactly as k_backsub does on the latency path; k_decide (shared) is the only writer of cur and flips it when, and only
// when, it accepts the candidate; the closing k_decide launch copies the state to FinalRec, which the host keeps in fin[w].s.
// xp / xl (and xv, xba, xbg) at fin[w].s.cur are therefore the accepted state of window w on either path — the buffer get_deltas
// reads. (ii) The kernels here read the window's arrays, the observation arrays and the Tile / tile_lmk lists only; layout_build
// fills those for both paths (the throughput path adds chunk tables beside them, it replaces nothing).
// Nothing of the solve is touched. Part of the library's single translation unit (ba_capi.hip); not a public header.
#pragma once
#include "cov_batch_kernels.h"
#include "cov_driver.h"
#include "covb_long_plan.h"

namespace {

struct CovbUnit {
    int w = 0;
    CovRoutes R;
    int route = COVB_ROUTE_NONE;
    size_t bytes = 0;                             // work arrays of the unit, what the scratch budget counts
    size_t nl = 1, no = 1, nn = 1;                // landmarks, observations, N_p^2 (at least 1 each)
    size_t r_lout = 0, r_size = 0, r_off = 0;     // doubles: its landmark table | its result block | where that starts among the call's
};
// A unit's result block, one piece of device memory copied to the host in one go with its group's: Sigma_pp [nn] | lout [r_lout] |
// landmark status [nl ints] | pivot flag [1 int]
// l0 / n_long: the long tracks of the call's units in front of the group | of the group's units (rows of its work table)
struct CovbGroup { int u0 = 0, u1 = 0; size_t doubles = 0, ints = 0, r_doubles = 0, r0 = 0; int l0 = 0, n_long = 0; };
// The group's work table of long tracks on the device (covb_long_plan.h), from covb_assemble to covb_landmarks; n_rows = 0: none
struct CovbLong { const int* d_rows = nullptr; int n_rows = 0, max_kf = 0; };

// 1. State and arguments, with the codes and the order of sadvio_ba_covariance (a batch the throughput kernels solved is served: see
// above). Host work only; nothing is written on an error.
int covb_check(sadvio_ba_handle* h, int n_item, const sadvio_cov_batch_item* items) {
    if (h->world > 1) return cov_invalid(h, "covariance_batch", ": the window is sharded over several GPUs (each rank holds a landmark partition only)");
    if (int rc = entry_state(h, "covariance_batch", NOT_DEFERRED | NEED_SOLVED)) return rc;
    if (n_item < 0) return cov_invalid(h, "covariance_batch", ": negative item count");
    if (n_item > 0 && !items) return cov_invalid(h, "covariance_batch", ": null items");
    for (int it = 0; it < n_item; it++)
        if (int rc = cov_check_request(h, "covariance_batch", items[it].w, &items[it].rq, true)) return rc;
    return SADVIO_OK;
}

// Does item I go through the single call's steps (cov_driver.h: cov_steps)? The DENSE, BAND and BORDER routes; under SADVIO_COV_SQRT=1 a
// NONE item too, for the landmark-block formula of the square-root assembly.
bool covb_single(const sadvio_ba_handle* h, const sadvio_cov_batch_item& I) {
    return I.route == SADVIO_COV_ROUTE_DENSE || I.route == SADVIO_COV_ROUTE_BAND || I.route == SADVIO_COV_ROUTE_BORDER || (I.route == SADVIO_COV_ROUTE_NONE && h->env.cov_sqrt == 1);
}

// 2. The route of every item; one unit per window that does not take the dense route
void covb_routes(sadvio_ba_handle* h, int n_item, sadvio_cov_batch_item* items, std::vector<CovbUnit>& units, std::vector<int>& unit_of) {
    std::vector<int> of_win(h->plan.wins.size(), -1);
    unit_of.assign((size_t)n_item, -1);
    for (int it = 0; it < n_item; it++) {
        sadvio_cov_batch_item& I = items[it];
        const WinDev& d = h->plan.wins[I.w].d;
        I.status = SADVIO_OK; I.n_lmk_singular = 0;
        const bool lds = h->env.cov_batch_lds != 0 && h->env.cov_sqrt != 1;   // (the square-root assembly has no group kernels: its items go one by one)
        I.route = d.Np == 0 ? SADVIO_COV_ROUTE_NONE : (d.Np <= COVB_CAP && lds ? SADVIO_COV_ROUTE_LDS : SADVIO_COV_ROUTE_DENSE);
        if (cov_band_route(h, I.w)) I.route = SADVIO_COV_ROUTE_BAND;   // (cov_driver.h: by default only a window the dense route refuses)
        if (cov_border_route(h, I.w)) I.route = SADVIO_COV_ROUTE_BORDER;   // (cov_driver.h: by default only a window that is refused otherwise)
        if (covb_single(h, I)) continue;
        const CovRoutes R = cov_routes(h, I.w, &I.rq, I.lmk_cov);
        if (of_win[I.w] < 0) {
            of_win[I.w] = (int)units.size();
            CovbUnit U;
            U.w = I.w; U.R = R; U.R.want_lmk = false; U.route = I.route;
            U.nl = (size_t)std::max(d.n_lmk, 1); U.no = (size_t)std::max(d.n_obs, 1); U.nn = (size_t)std::max(d.Np, 1) * std::max(d.Np, 1);
            U.bytes = sizeof(double) * (21 * U.nl + (COV_ENT_W + COV_ENT_HPP) * U.no + 2 * U.nn) + sizeof(int) * (2 * U.nl + U.no + 1);
            if (R.n_long > 0) U.bytes += sizeof(int) * U.nl;   // CovDev::is_long
            units.push_back(U);
        }
        CovbUnit& U = units[of_win[I.w]];
        U.R.want_lmk |= R.want_lmk;
        unit_of[it] = of_win[I.w];
    }
}

// An item above the cap: the steps of sadvio_ba_covariance, unchanged, with their choice of assembly and their retry (cov_check's
// tests were made for every item by covb_check)
int covb_dense_item(sadvio_ba_handle* h, sadvio_cov_batch_item& I) {
    const int rc = cov_steps(h, I.w, cov_routes(h, I.w, &I.rq, I.lmk_cov), cov_read_back_into(h, I.w, &I.rq, I.kf_cov, I.pair_cov, I.lmk_cov, &I.n_lmk_singular));
    if (rc == SADVIO_E_NOT_USABLE) { I.status = SADVIO_E_NOT_USABLE; return SADVIO_OK; }
    return rc;
}

// An LDS item whose unit failed the pivot test, SADVIO_COV_SQRT unset: once more on its own through the single call's steps with the
// square-root assembly, before SADVIO_E_NOT_USABLE is written
int covb_retry_item(sadvio_ba_handle* h, sadvio_cov_batch_item& I) {
    CovRoutes R = cov_routes(h, I.w, &I.rq, I.lmk_cov);
    R.sqrt = true;
    const int rc = cov_attempt(h, I.w, R, cov_read_back_into(h, I.w, &I.rq, I.kf_cov, I.pair_cov, I.lmk_cov, &I.n_lmk_singular));
    if (rc == SADVIO_E_NOT_USABLE) return SADVIO_OK;
    if (rc == SADVIO_OK) I.status = SADVIO_OK;
    return rc;
}

// 3. Groups of consecutive units under the scratch budget (a unit larger than the budget is a group of its own); the pools, the
// unit table and the pinned block are sized once, for the largest group and for all results, before anything is launched
int covb_groups(sadvio_ba_handle* h, std::vector<CovbUnit>& units, std::vector<CovbGroup>& groups) {
    CovBatchScratch& B = h->cvb;
    const size_t budget = (size_t)std::max(h->env.cov_batch_scratch_mb, 0) << 20;
    size_t used = 0, max_d = 1, max_i = 1, max_r = 1, r_tot = 0;
    int l_tot = 0;
    for (int u = 0; u < (int)units.size(); u++) {
        CovbUnit& U = units[u];
        if (groups.empty() || used + U.bytes > budget) { groups.push_back(CovbGroup{u, u, 0, 0, 0, r_tot, l_tot, 0}); used = 0; }
        CovbGroup& g = groups.back();
        U.r_lout = U.R.want_lmk ? 9 * U.nl : 0;
        U.r_size = U.nn + U.r_lout + (U.nl + 1) / 2 + 1;
        U.r_off = r_tot; r_tot += U.r_size;
        g.u1 = u + 1; g.doubles += 12 * U.nl + (COV_ENT_W + COV_ENT_HPP) * U.no + U.nn; g.ints += U.nl + U.no; g.r_doubles += U.r_size;
        if (U.R.n_long > 0) { g.ints += U.nl; g.n_long += U.R.n_long; l_tot += U.R.n_long; }
        used += U.bytes;
        max_d = std::max(max_d, g.doubles); max_i = std::max(max_i, g.ints); max_r = std::max(max_r, g.r_doubles);
    }
    HIP_TRY(B.pool.alloc(max_d)); HIP_TRY(B.ipool.alloc(max_i)); HIP_TRY(B.rpool.alloc(max_r));
    HIP_TRY(B.ptab.alloc((size_t)h->plan.n_kf_tot * POSE_TAB));
    // the tables, group after group: a group's units, then its long tracks' rows (8 bytes each: what follows stays aligned)
    static_assert(sizeof(int) * COVB_LONG_ROW == 8 && sizeof(CovUnit) % 8 == 0, "the tables are laid out back to back");
    B.tab_bytes = sizeof(CovUnit) * units.size() + sizeof(int) * COVB_LONG_ROW * (size_t)l_tot;
    HIP_TRY(B.units.alloc(B.tab_bytes));
    HIP_TRY(B.pin(B.tab_bytes + sizeof(double) * r_tot));
    return SADVIO_OK;
}

// where group g's tables start in the pinned block and in CovBatchScratch::units
size_t covb_tab_offset(const CovbGroup& g) { return sizeof(CovUnit) * (size_t)g.u0 + sizeof(int) * COVB_LONG_ROW * (size_t)g.l0; }

// the call's result blocks in the pinned block, behind the tables
double* covb_host_results(sadvio_ba_handle* h, const std::vector<CovbUnit>&) { return (double*)(h->cvb.pinned + h->cvb.tab_bytes); }

// 4. One group: the unit table and the work table of its long tracks; linearise every unit at its x*; every S, full symmetric
int covb_assemble(sadvio_ba_handle* h, const std::vector<CovbUnit>& units, const CovbGroup& g, const DevPtrs& P, const CovUnit*& d_units, CovbLong& L) {
    CovBatchScratch& B = h->cvb;
    const int nu = g.u1 - g.u0;
    CovUnit* tab = (CovUnit*)(B.pinned + covb_tab_offset(g));
    // the work pool: every S of the group first (one memset), then unit after unit; the result pool: block after block
    size_t s_tot = 0;
    for (int u = g.u0; u < g.u1; u++) s_tot += units[u].nn;
    double* pd = B.pool.p + s_tot; double* ps = B.pool.p;
    int* pi = B.ipool.p;
    size_t i_tot = 0;   // (the is_long arrays of the units with long tracks lie behind every other int array: one memset)
    for (int u = g.u0; u < g.u1; u++) i_tot += units[u].nl + units[u].no;
    int* const pl0 = B.ipool.p + i_tot;
    int* pl = pl0;
    std::vector<int> lb((size_t)nu), le((size_t)nu);
    int mx_tab = 1, mx_tiles = 0, mx_schur = 0, mx_dense = 0;
    bool any_kept = false, any_np = false;
    for (int u = g.u0; u < g.u1; u++) {
        const CovbUnit& U = units[u];
        const WinDev& d = h->plan.wins[U.w].d;
        const size_t nl = U.nl, no = U.no, nn = U.nn;
        CovUnit& T = tab[u - g.u0];
        memset(&T, 0, sizeof(T));
        CovDev& C = T.C;
        C.w = U.w; C.cur = U.R.cur; C.Np = U.R.Np; C.huber_a = h->cov_huber_a;
        C.ptab = B.ptab.p;
        C.S = ps; ps += nn;
        C.hll = pd; pd += 6 * nl; C.hinv = pd; pd += 6 * nl;
        C.ent_w = pd; pd += COV_ENT_W * no; C.ent_hpp = pd; pd += COV_ENT_HPP * no;
        C.ent_n = pi; pi += nl; C.ent_col = pi; pi += no;
        if (U.R.n_long > 0) { C.is_long = pl; pl += nl; }
        lb[u - g.u0] = U.R.long_first; le[u - g.u0] = U.R.long_first + U.R.n_long;
        double* pr = B.rpool.p + (U.r_off - g.r0);
        T.sig = pr; C.Sig = pr; C.lout = pr + nn;
        C.status = (int*)(pr + nn + U.r_lout);
        T.bad = C.status + 2 * ((nl + 1) / 2);
        T.route = U.route;
        T.G = U.R.want_lmk && d.n_lmk > 0 ? U.R.G : 0;
        mx_tab = std::max(mx_tab, (std::max(d.n_kf, d.n_lmk) + 255) / 256);
        mx_tiles = std::max(mx_tiles, d.tile_end - d.tile_begin);
        if (U.R.Np > 0) {
            any_np = true;
            mx_schur = std::max(mx_schur, d.n_free_kf * (d.n_free_kf + 1) / 2);
            any_kept |= U.R.kept;
            if (U.R.dense) mx_dense = std::max(mx_dense, (int)(((long long)d.dp_n * d.dp_n + 255) / 256));
        }
    }
    CovbLongPlan lp;
    covb_long_plan(nu, lb.data(), le.data(), h->plan.long_rec.data(), LONG_REC, lp);
    assert(lp.n_rows() == g.n_long);
    if (lp.n_rows() > 0) memcpy(tab + nu, lp.rows.data(), sizeof(int) * lp.rows.size());
    d_units = (const CovUnit*)(B.units.p + covb_tab_offset(g));
    L = CovbLong{(const int*)(d_units + nu), lp.n_rows(), lp.max_kf};
    HIP_TRY(hipMemcpyAsync((void*)d_units, tab, sizeof(CovUnit) * nu + sizeof(int) * lp.rows.size(), hipMemcpyHostToDevice, h->stream));
    HIP_TRY(hipMemsetAsync(B.pool.p, 0, sizeof(double) * s_tot, h->stream));
    if (pl > pl0) HIP_TRY(hipMemsetAsync(pl0, 0, sizeof(int) * (size_t)(pl - pl0), h->stream));
    const bool pix = h->plan.factor_type == SADVIO_FACTOR_PIXEL;
    ScopedTimer t(h, "covb_assemble");
    hipLaunchKernelGGL(k_covb_tables, dim3(mx_tab, nu), dim3(256), 0, h->stream, P, d_units, B.ptab.p);
    if (mx_tiles > 0) hipLaunchKernelGGL(pix ? k_covb_assemble<0> : k_covb_assemble<1>, dim3(mx_tiles, nu), dim3(COV_THREADS), 0, h->stream, P, d_units);
    if (L.n_rows > 0) {   // the long tracks into the tables the tile walk just filled, in front of k_covb_schur
        LongArgs A = cov_long_args(h);
        A.max_kf = L.max_kf;
        ScopedTimer tl(h, "k_covb_long");
        hipLaunchKernelGGL(pix ? k_covb_long<0> : k_covb_long<1>, dim3(L.n_rows), dim3(LONG_THREADS), cov_long_lds_bytes(L.max_kf), h->stream, P, d_units, L.d_rows, A);
    }
    if (any_np) {
        if (mx_schur > 0) hipLaunchKernelGGL(k_covb_schur, dim3(mx_schur, nu), dim3(COV_SCHUR_THREADS), 0, h->stream, P, d_units);
        if (any_kept) hipLaunchKernelGGL(pix ? k_covb_kept<0> : k_covb_kept<1>, dim3(nu), dim3(64), 0, h->stream, P, d_units);
        hipLaunchKernelGGL(k_covb_factors, dim3(nu), dim3(64), 0, h->stream, P, d_units);
        if (mx_dense > 0) hipLaunchKernelGGL(k_covb_dense, dim3(mx_dense, nu), dim3(256), 0, h->stream, P, d_units);
    }
    HIP_TRY(hipGetLastError());
    return SADVIO_OK;
}

// 5. Sigma_pp of every unit of the group with N_p > 0: one workgroup each, in LDS. A failed pivot test sets the unit's flag on the
// device; the host reads it behind the call's one wait.
int covb_invert(sadvio_ba_handle* h, const std::vector<CovbUnit>& units, const CovbGroup& g, const CovUnit* d_units) {
    int nb = 0;
    for (int u = g.u0; u < g.u1; u++)
        if (units[u].route == COVB_ROUTE_LDS) nb = std::max(nb, (units[u].R.Np + 15) / 16);
    if (nb == 0) return SADVIO_OK;
    (void)hipFuncSetAttribute((const void*)k_cov_inv_lds, hipFuncAttributeMaxDynamicSharedMemorySize, covb_lds_bytes(COVB_CAP / 16));
    ScopedTimer t(h, "k_cov_inv_lds");
    hipLaunchKernelGGL(k_cov_inv_lds, dim3(g.u1 - g.u0), dim3(COVB_THREADS), covb_lds_bytes(nb), h->stream, d_units);
    HIP_TRY(hipGetLastError());
    return SADVIO_OK;
}

// 6. Sigma_ll of every landmark of the units that were asked for landmark blocks; then the group's results on their way to the host
int covb_landmarks(sadvio_ba_handle* h, const std::vector<CovbUnit>& units, const CovbGroup& g, const DevPtrs& P, const CovUnit* d_units, const CovbLong& L) {
    CovBatchScratch& B = h->cvb;
    const int nu = g.u1 - g.u0;
    int blocks[2] = {0, 0};   // G = 16 | 64
    for (int u = g.u0; u < g.u1; u++) {
        const CovbUnit& U = units[u];
        const WinDev& d = h->plan.wins[U.w].d;
        if (!U.R.want_lmk || d.n_lmk == 0) continue;
        const int per = COV_THREADS / U.R.G;
        int& b = blocks[U.R.G == 16 ? 0 : 1];
        b = std::max(b, (d.n_lmk + per - 1) / per);
    }
    {
        ScopedTimer t(h, "k_covb_lmk");
        if (blocks[0]) hipLaunchKernelGGL(k_covb_lmk<16>, dim3(blocks[0], nu), dim3(COV_THREADS), 0, h->stream, P, d_units);
        if (blocks[1]) hipLaunchKernelGGL(k_covb_lmk<64>, dim3(blocks[1], nu), dim3(COV_THREADS), 0, h->stream, P, d_units);
    }
    if (L.n_rows > 0 && (blocks[0] || blocks[1])) {   // the long tracks' blocks, which k_covb_lmk skipped (CovDev::is_long)
        LongArgs A = cov_long_args(h);
        A.max_kf = L.max_kf;
        ScopedTimer tl(h, "k_covb_lmk_long");
        hipLaunchKernelGGL(k_covb_lmk_long, dim3(L.n_rows), dim3(LONG_THREADS), 0, h->stream, P, d_units, L.d_rows, A);
    }
    HIP_TRY(hipGetLastError());
    HIP_TRY(hipMemcpyAsync(covb_host_results(h, units) + g.r0, B.rpool.p, sizeof(double) * g.r_doubles, hipMemcpyDeviceToHost, h->stream));
    return SADVIO_OK;
}

// 7. The call's one wait; every item's blocks are picked from its unit's Sigma_pp and landmark table on the host, as cov_read_back
// picks them. An item whose unit failed the pivot test gets its status and nothing else.
int covb_read_back(sadvio_ba_handle* h, int n_item, sadvio_cov_batch_item* items, const std::vector<CovbUnit>& units, const std::vector<int>& unit_of) {
    if (int rc = cov_wait(h)) return rc;
    for (int it = 0; it < n_item; it++) {
        if (unit_of[it] < 0) continue;
        sadvio_cov_batch_item& I = items[it];
        const CovbUnit& U = units[unit_of[it]];
        const double* sig = covb_host_results(h, units) + U.r_off;
        const double* lo = sig + U.nn;
        const int* st = (const int*)(lo + U.r_lout);
        if (st[2 * ((U.nl + 1) / 2)] != 0) { I.status = SADVIO_E_NOT_USABLE; continue; }
        const WinDev& d = h->plan.wins[I.w].d;
        cov_pick_blocks(h->plan, d, &I.rq, sig, U.R.Np, I.kf_cov, I.pair_cov);
        cov_pick_landmarks(&I.rq, d, lo, st, I.lmk_cov, &I.n_lmk_singular);
    }
    return SADVIO_OK;
}

int covb_run(sadvio_ba_handle* h, int n_item, sadvio_cov_batch_item* items) {
    if (int rc = covb_check(h, n_item, items)) return rc;
    if (n_item == 0) return SADVIO_OK;
    HIP_TRY(hipSetDevice(h->device));
    std::vector<CovbUnit> units;
    std::vector<int> unit_of;
    covb_routes(h, n_item, items, units, unit_of);
    for (int it = 0; it < n_item; it++)
        if (covb_single(h, items[it]))
            if (int rc = covb_dense_item(h, items[it])) return rc;
    if (units.empty()) return SADVIO_OK;
    std::vector<CovbGroup> groups;
    if (int rc = covb_groups(h, units, groups)) return rc;
    SolveOpts so{};
    so.huber_a = h->cov_huber_a;
    const DevPtrs P = make_ptrs(h, so, h->last_slots + 2);
    for (const CovbGroup& g : groups) {
        const CovUnit* d_units = nullptr;
        CovbLong L;
        if (int rc = covb_assemble(h, units, g, P, d_units, L)) return rc;
        if (int rc = covb_invert(h, units, g, d_units)) return rc;
        if (int rc = covb_landmarks(h, units, g, P, d_units, L)) return rc;
    }
    if (int rc = covb_read_back(h, n_item, items, units, unit_of)) return rc;
    if (h->env.cov_sqrt != 0)
        for (int it = 0; it < n_item; it++)
            if (unit_of[it] >= 0 && items[it].status == SADVIO_E_NOT_USABLE)
                if (int rc = covb_retry_item(h, items[it])) return rc;
    return SADVIO_OK;
}

}  // namespace
