// ba_capi.hip — host driver + C ABI (include/sadvio_ba.h) of the MI355X BA backend.
//
// Replaces, behind the reference's optimizer boundary, the body of AOptimizer::localMapBA /
// localMapVIOptimization from `ceres::Solve` on (AOptimizer.cpp:326,388): the windows are uploaded
// once (set_windows), the whole LM solve is enqueued on the handle's stream without host round
// trips, and deltas are read back for the adapter to apply (AOptimizer.cpp:329-340).
// There is no CPU fallback: without a gfx950 device every compute call fails.
#include "ba_handle.h"
#include "solve_driver.h"
#include "layout_driver.h"

namespace {
// why sadvio_ba_create refused its configuration: there is no handle to hold the text, sadvio_ba_last_error(NULL) returns it
thread_local std::string create_err;
}  // namespace

extern "C" {

int sadvio_ba_device_count(void) {
    int n = 0;
    if (hipGetDeviceCount(&n) != hipSuccess) return 0;
    int ok = 0;
    for (int i = 0; i < n; i++) {
        hipDeviceProp_t p;
        if (hipGetDeviceProperties(&p, i) == hipSuccess && strstr(p.gcnArchName, "gfx950")) ok++;
    }
    return ok;
}

void sadvio_ba_default_options(sadvio_solve_options* o) {
    if (!o) return;
    memset(o, 0, sizeof(*o));
    o->max_num_iterations = 20;   // AOptimizer.cpp:319
    o->function_tolerance = 1e-3; // AOptimizer.cpp:322
    // everything the reference leaves unset: Ceres Solver 2.2.0 defaults
    o->jacobi_scaling = 1;
    o->max_num_consecutive_invalid_steps = 5;
    o->gradient_tolerance = 1e-10;
    o->parameter_tolerance = 1e-8;
    o->initial_trust_region_radius = 1e4;
    o->max_trust_region_radius = 1e16;
    o->min_trust_region_radius = 1e-32;
    o->min_lm_diagonal = 1e-6;
    o->max_lm_diagonal = 1e32;
    o->min_relative_decrease = 1e-3;
}

int sadvio_ba_create(const sadvio_ba_config* cfg, sadvio_ba_handle** out) {
    if (!out) return SADVIO_E_INVALID_ARG;
    *out = nullptr;
    create_err.clear();
    if (cfg && (cfg->reserved & SADVIO_CFG_LONG_TRACK_PRIORS) && !(cfg->reserved & SADVIO_CFG_LONG_TRACKS)) {
        create_err = "create: SADVIO_CFG_LONG_TRACK_PRIORS needs SADVIO_CFG_LONG_TRACKS (a handle without the long path has no long track to carry a prior on)";
        return SADVIO_E_INVALID_ARG;
    }
    if (cfg && (cfg->reserved & SADVIO_CFG_LONG_TRACK_COVARIANCE) && !(cfg->reserved & SADVIO_CFG_LONG_TRACKS)) {
        create_err = "create: SADVIO_CFG_LONG_TRACK_COVARIANCE needs SADVIO_CFG_LONG_TRACKS (a handle without the long path has no long track to form a covariance of)";
        return SADVIO_E_INVALID_ARG;
    }
    if (cfg && (cfg->reserved & SADVIO_CFG_LONG_TRACK_BATCH) && !(cfg->reserved & SADVIO_CFG_LONG_TRACKS)) {
        create_err = "create: SADVIO_CFG_LONG_TRACK_BATCH needs SADVIO_CFG_LONG_TRACKS (a handle without the long path has no long track for a batch call to serve)";
        return SADVIO_E_INVALID_ARG;
    }
    int n = 0;
    if (hipGetDeviceCount(&n) != hipSuccess || n == 0) return SADVIO_E_NO_DEVICE;
    int dev = cfg ? cfg->device : 0;
    if (dev < 0 || dev >= n) return SADVIO_E_INVALID_ARG;
    hipDeviceProp_t prop;
    if (hipGetDeviceProperties(&prop, dev) != hipSuccess) return SADVIO_E_HIP;
    if (!strstr(prop.gcnArchName, "gfx950")) return SADVIO_E_NO_DEVICE;  // kernels are built for gfx950 only
    if (hipSetDevice(dev) != hipSuccess) return SADVIO_E_HIP;
    auto* h = new sadvio_ba_handle();
    h->env.read();
    h->up.trace = (h->env.debug & 8192) != 0;
    if (cfg) h->cfg = *cfg;
    // long tracks are served by handles that ask for them: every other handle refuses a 65th observation as it always did
    if (h->cfg.reserved & SADVIO_CFG_LONG_TRACKS) h->env.long_min = h->env.long_min_env ? h->env.long_min_env : MAX_LMK_OBS + 1;
    // ... and marginalised, sparsified and held by priors on handles that ask for that as well: every other handle keeps those refusals
    h->env.long_priors = (h->cfg.reserved & SADVIO_CFG_LONG_TRACK_PRIORS) != 0;
    // ... and asked for covariances (the single call and the cross call) on handles that ask for that: independent of the priors' flag
    h->env.long_cov = (h->cfg.reserved & SADVIO_CFG_LONG_TRACK_COVARIANCE) != 0;
    // ... and the relative marginalisations, and with the covariance flag covariance_batch, on handles that ask for that
    h->env.long_batch = (h->cfg.reserved & SADVIO_CFG_LONG_TRACK_BATCH) != 0;
    h->device = dev;
    if (hipStreamCreateWithFlags(&h->stream, hipStreamNonBlocking) != hipSuccess) { delete h; return SADVIO_E_HIP; }
    if (hipStreamCreateWithFlags(&h->side, hipStreamNonBlocking) != hipSuccess) h->side = nullptr;   // optional: without it everything is serial
    for (hipEvent_t* e : {&h->ev_fork, &h->ev_lin, &h->ev_solved, &h->ev_cost})
        if (hipEventCreateWithFlags(e, hipEventDisableTiming) != hipSuccess) { *e = nullptr; if (h->side) { (void)hipStreamDestroy(h->side); h->side = nullptr; } }
    *out = h;
    return SADVIO_OK;
}

void sadvio_ba_destroy(sadvio_ba_handle* h) {
    if (!h) return;
    (void)hipSetDevice(h->device);
    if (h->stream) { (void)hipStreamSynchronize(h->stream); }
    if (h->graph_exec) (void)hipGraphExecDestroy(h->graph_exec);
    if (h->rccl.comm) (void)h->rccl.destroy(h->rccl.comm);
    if (h->h_final) (void)hipHostFree(h->h_final);
    if (h->h_deltas) (void)hipHostFree(h->h_deltas);
    if (h->side) { (void)hipStreamSynchronize(h->side); (void)hipStreamDestroy(h->side); }
    for (hipEvent_t e : {h->ev_fork, h->ev_lin, h->ev_solved, h->ev_cost}) if (e) (void)hipEventDestroy(e);
    if (h->stream) (void)hipStreamDestroy(h->stream);
    for (auto& e : h->ev_pool) { (void)hipEventDestroy(e.first); (void)hipEventDestroy(e.second); }
    delete h;
}

int sadvio_ba_set_windows(sadvio_ba_handle* h, int32_t n_windows, const sadvio_flat_window* wins) {
    if (!h) return SADVIO_E_INVALID_ARG;
    if (n_windows <= 0 || !wins) { h->err = "set_windows: no windows"; return SADVIO_E_INVALID_ARG; }
    h->uploaded = false; h->solved = false;
    for (int w = 0; w < n_windows; w++) {
        const int rc = check_flat_window(wins[w], w, h->err);
        if (rc != SADVIO_OK) return rc;
    }
    // deep copies: later set_* calls rebuild the layout without the caller's buffers
    if ((int)h->src.size() != n_windows) h->src.assign(n_windows, SrcWin());   // same batch size: the copies below reuse their capacity
    for (int w = 0; w < n_windows; w++) {
        const sadvio_flat_window& F = wins[w];
        SrcWin& S = h->src[w];
        S.cam_sigma.clear(); S.kf_id.clear(); S.kf_const.clear(); S.kf_vel.clear(); S.kf_ba.clear(); S.kf_bg.clear();
        S.lmk_p.clear(); S.lmk_id.clear(); S.lmk_const.clear(); S.obs_kf.clear(); S.obs_cam.clear(); S.obs_meas.clear();
        S.a_src.clear();
        const int ms = F.factor_type == SADVIO_FACTOR_PIXEL ? 2 : 3;
        S.kf_T.assign(F.kf_T_f_w, F.kf_T_f_w + 12 * (size_t)F.n_kf);
        S.cam_K.assign(F.cam_K, F.cam_K + 4 * (size_t)F.n_cam); S.cam_T.assign(F.cam_T_s_f, F.cam_T_s_f + 12 * (size_t)F.n_cam);
        if (F.cam_sigma) S.cam_sigma.assign(F.cam_sigma, F.cam_sigma + F.n_cam);
        if (F.kf_id) S.kf_id.assign(F.kf_id, F.kf_id + F.n_kf);
        if (F.kf_const) S.kf_const.assign(F.kf_const, F.kf_const + F.n_kf);
        if (F.kf_vel) S.kf_vel.assign(F.kf_vel, F.kf_vel + 3 * (size_t)F.n_kf);
        if (F.kf_ba) S.kf_ba.assign(F.kf_ba, F.kf_ba + 3 * (size_t)F.n_kf);
        if (F.kf_bg) S.kf_bg.assign(F.kf_bg, F.kf_bg + 3 * (size_t)F.n_kf);
        if (F.n_lmk) { S.lmk_p.assign(F.lmk_p, F.lmk_p + 3 * (size_t)F.n_lmk); S.lmk_obs_ptr.assign(F.lmk_obs_ptr, F.lmk_obs_ptr + F.n_lmk + 1); }
        else S.lmk_obs_ptr.assign(1, 0);
        if (F.lmk_id) S.lmk_id.assign(F.lmk_id, F.lmk_id + F.n_lmk);
        if (F.lmk_const) S.lmk_const.assign(F.lmk_const, F.lmk_const + F.n_lmk);
        if (F.n_obs) {
            S.obs_kf.assign(F.obs_kf, F.obs_kf + F.n_obs); S.obs_cam.assign(F.obs_cam, F.obs_cam + F.n_obs);
            S.obs_meas.assign(F.obs_meas, F.obs_meas + (size_t)ms * F.n_obs);
        }
        S.v = F;
        S.v.kf_T_f_w = S.kf_T.data(); S.v.cam_K = S.cam_K.data(); S.v.cam_T_s_f = S.cam_T.data();
        S.v.cam_sigma = F.cam_sigma ? S.cam_sigma.data() : nullptr;
        S.v.kf_id = F.kf_id ? S.kf_id.data() : nullptr; S.v.kf_const = F.kf_const ? S.kf_const.data() : nullptr;
        S.v.kf_vel = F.kf_vel ? S.kf_vel.data() : nullptr; S.v.kf_ba = F.kf_ba ? S.kf_ba.data() : nullptr; S.v.kf_bg = F.kf_bg ? S.kf_bg.data() : nullptr;
        S.v.lmk_p = S.lmk_p.data(); S.v.lmk_obs_ptr = S.lmk_obs_ptr.data();
        S.v.lmk_id = F.lmk_id ? S.lmk_id.data() : nullptr; S.v.lmk_const = F.lmk_const ? S.lmk_const.data() : nullptr;
        S.v.obs_kf = S.obs_kf.data(); S.v.obs_cam = S.obs_cam.data(); S.v.obs_meas = S.obs_meas.data();
    }
    h->priors_per_win.assign(n_windows, {});
    h->imus_per_win.assign(n_windows, {});
    h->dprior_per_win.assign(n_windows, {});
    h->sparse_per_win.assign(n_windows, {});
    h->lines_per_win.assign(n_windows, {});
    if (h->defer) {
        // the factor setters that follow validate against the windows' sizes and convert indices with their offsets in the batch:
        // stub records with the numbers layout_build derives at commit (the cameras are not de-duplicated yet: no setter reads them)
        layout_windows(n_windows, wins, h->plan);
        h->uploaded = true; h->pending = true;
        return SADVIO_OK;
    }
    return layout_build(h);
}

int sadvio_ba_begin_update(sadvio_ba_handle* h) {
    if (!h) return SADVIO_E_INVALID_ARG;
    h->defer = true; h->pending = false;
    return SADVIO_OK;
}

int sadvio_ba_commit_update(sadvio_ba_handle* h) {
    if (!h) return SADVIO_E_INVALID_ARG;
    if (!h->defer) { h->err = "commit_update without begin_update"; return SADVIO_E_STATE; }
    h->defer = false;
    if (!h->pending) return SADVIO_OK;
    h->pending = false;
    return layout_build(h);   // (a failed build leaves the handle without a layout: the deferred set_windows left stub window records)
}

int sadvio_ba_set_lines(sadvio_ba_handle* h, int32_t w, const sadvio_line_set* L) {
    if (!h) return SADVIO_E_INVALID_ARG;
    if (!h->uploaded) { h->err = "set_lines before set_windows"; return SADVIO_E_STATE; }
    if (w < 0 || w >= (int)h->plan.wins.size()) { h->err = "set_lines: window out of range"; return SADVIO_E_INVALID_ARG; }
    const int n = L ? L->n_line : 0;
    if (h->world > 1 && n > 0) { h->err = "set_lines: not supported on a window sharded over several GPUs"; return SADVIO_E_INVALID_ARG; }
    HIP_TRY(hipSetDevice(h->device));
    const WinDev& d = h->plan.wins[w].d;
    LineSetHost H;
    if (n > 0) {
        if (n < 0 || L->n_obs < 0 || !L->line_T_w_l || !L->line_model || !L->line_obs_ptr || (L->n_obs > 0 && (!L->obs_kf || !L->obs_cam || !L->obs_meas))) {
            h->err = "set_lines: missing array"; return SADVIO_E_INVALID_ARG;
        }
        if (L->line_obs_ptr[0] != 0 || L->line_obs_ptr[n] != L->n_obs) { h->err = "set_lines: line_obs_ptr is not a CSR over n_obs"; return SADVIO_E_INVALID_ARG; }
        for (int l = 0; l < n; l++) if (L->line_obs_ptr[l + 1] < L->line_obs_ptr[l]) { h->err = "set_lines: CSR not monotone"; return SADVIO_E_INVALID_ARG; }
        for (int o = 0; o < L->n_obs; o++)
            if (L->obs_kf[o] < 0 || L->obs_kf[o] >= d.n_kf || L->obs_cam[o] < 0 || L->obs_cam[o] >= h->src[w].v.n_cam) {   // the caller's camera count (cam_map, built with the layout, has as many entries)
                h->err = "set_lines: observation index out of range"; return SADVIO_E_INVALID_ARG;
            }
        const int ms = d.factor_type == SADVIO_FACTOR_PIXEL ? 4 : 6;
        H.id.resize(n);
        for (int l = 0; l < n; l++) H.id[l] = L->line_id ? L->line_id[l] : l;
        H.T.assign(L->line_T_w_l, L->line_T_w_l + 12 * (size_t)n); H.model.assign(L->line_model, L->line_model + 6 * (size_t)n);
        if (L->line_const) H.is_const.assign(L->line_const, L->line_const + n);
        H.ptr.assign(L->line_obs_ptr, L->line_obs_ptr + n + 1);
        if (L->n_obs) {
            H.obs_kf.assign(L->obs_kf, L->obs_kf + L->n_obs); H.obs_cam.assign(L->obs_cam, L->obs_cam + L->n_obs);
            H.meas.assign(L->obs_meas, L->obs_meas + (size_t)ms * L->n_obs);
        }
    }
    h->lines_per_win[w] = std::move(H);
    h->solved = false;
    if (h->defer) { h->pending = true; return SADVIO_OK; }
    h->up.reset();
    int rc = layout_reduced(h);   // the lines enlarge the reduced system; the landmark tiles are unchanged
    if (rc != SADVIO_OK) return rc;
    if (h->defer) { h->pending = true; return SADVIO_OK; }
    return upload_priors(h);
}

int sadvio_ba_get_line_deltas(sadvio_ba_handle* h, int32_t w, double* line_delta6) {
    if (!h) return SADVIO_E_INVALID_ARG;
    if (!h->solved) { h->err = "get_line_deltas before solve"; return SADVIO_E_STATE; }
    if (w < 0 || w >= (int)h->plan.wins.size() || !line_delta6) { h->err = "get_line_deltas: bad argument"; return SADVIO_E_INVALID_ARG; }
    HIP_TRY(hipSetDevice(h->device));
    const WinDev& d = h->plan.wins[w].d;
    const int n = d.line_end - d.line_begin;
    if (n > 0) HIP_TRY(hipMemcpy(line_delta6, h->d_xline.p + (size_t)h->fin[w].s.cur * 6 * h->n_line_tot + 6 * (size_t)d.line_begin, sizeof(double) * 6 * n, hipMemcpyDeviceToHost));
    return SADVIO_OK;
}

int sadvio_ba_set_pose_priors(sadvio_ba_handle* h, int32_t w, int32_t n, const sadvio_pose_prior* pr) {
    if (!h) return SADVIO_E_INVALID_ARG;
    if (!h->uploaded) { h->err = "set_pose_priors before set_windows"; return SADVIO_E_STATE; }
    if (w < 0 || w >= (int)h->plan.wins.size() || n < 0 || (n > 0 && !pr)) { h->err = "set_pose_priors: bad argument"; return SADVIO_E_INVALID_ARG; }
    HIP_TRY(hipSetDevice(h->device));
    auto& v = h->priors_per_win[w];
    v.clear();
    for (int i = 0; i < n; i++) {
        if (pr[i].kf < 0 || pr[i].kf >= h->plan.wins[w].d.n_kf) { h->err = "set_pose_priors: kf out of range"; return SADVIO_E_INVALID_ARG; }
        PriorDev d{};
        d.kf = h->plan.wins[w].d.kf_base + pr[i].kf;
        memcpy(d.T_prior, pr[i].T_prior, sizeof(d.T_prior));
        memcpy(d.inf, pr[i].inf_diag, sizeof(d.inf));
        v.push_back(d);
    }
    if (h->defer) { h->pending = true; return SADVIO_OK; }
    h->up.reset();
    return upload_priors(h);
}

// 9x9 square-root information W = L^T with L L^T = cov^-1 (residuals.hpp:151-154): Gauss-Jordan inverse with
// partial pivoting + Cholesky, on the host, once per factor.
static bool imu_sqrt_information(const double* cov, double* W) {
    double A[81], I[81];
    memcpy(A, cov, sizeof(A));
    memset(I, 0, sizeof(I));
    for (int i = 0; i < 9; i++) I[i * 9 + i] = 1.0;
    for (int c = 0; c < 9; c++) {
        int piv = c;
        double best = fabs(A[c * 9 + c]);
        for (int r = c + 1; r < 9; r++)
            if (fabs(A[r * 9 + c]) > best) { best = fabs(A[r * 9 + c]); piv = r; }
        if (best == 0.0) return false;
        if (piv != c)
            for (int j = 0; j < 9; j++) { std::swap(A[c * 9 + j], A[piv * 9 + j]); std::swap(I[c * 9 + j], I[piv * 9 + j]); }
        double d = 1.0 / A[c * 9 + c];
        for (int j = 0; j < 9; j++) { A[c * 9 + j] *= d; I[c * 9 + j] *= d; }
        for (int r = 0; r < 9; r++) {
            if (r == c) continue;
            double f = A[r * 9 + c];
            if (f == 0.0) continue;
            for (int j = 0; j < 9; j++) { A[r * 9 + j] -= f * A[c * 9 + j]; I[r * 9 + j] -= f * I[c * 9 + j]; }
        }
    }
    double L[81];
    memset(L, 0, sizeof(L));
    for (int j = 0; j < 9; j++) {
        double s = I[j * 9 + j];
        for (int k = 0; k < j; k++) s -= L[j * 9 + k] * L[j * 9 + k];
        if (!(s > 0.0)) return false;
        double d = sqrt(s);
        L[j * 9 + j] = d;
        for (int i = j + 1; i < 9; i++) {
            double t = I[i * 9 + j];
            for (int k = 0; k < j; k++) t -= L[i * 9 + k] * L[j * 9 + k];
            L[i * 9 + j] = t / d;
        }
    }
    for (int i = 0; i < 9; i++)
        for (int j = 0; j < 9; j++) W[i * 9 + j] = L[j * 9 + i];
    return true;
}

// exp_so3((a, b, 0)) row-major (geometry.h:131-147: first order below 1e-9)
static void host_exp_so3(double a, double b, double* R) {
    const double th = std::sqrt(a * a + b * b);
    const double I[9] = {1, 0, 0, 0, 1, 0, 0, 0, 1};
    if (th < 1e-9) { const double S[9] = {0, 0, b, 0, 0, -a, -b, a, 0}; for (int i = 0; i < 9; i++) R[i] = I[i] + S[i]; return; }
    const double x = a / th, y = b / th;
    const double S[9] = {0, 0, y, 0, 0, -x, -y, x, 0};
    double S2[9];
    for (int i = 0; i < 3; i++) for (int j = 0; j < 3; j++) S2[3 * i + j] = S[3 * i] * S[j] + S[3 * i + 1] * S[3 + j] + S[3 * i + 2] * S[6 + j];
    for (int i = 0; i < 9; i++) R[i] = I[i] + (1.0 - std::cos(th)) * S2[i] + std::sin(th) * S[i];
}
static bool make_imu_dev(const sadvio_imu_factor& f, int kf_base, ImuDev& o) {
    o.kf_i = kf_base + f.kf_i; o.kf_j = kf_base + f.kf_j; o.dt = f.dt;
    memcpy(o.dR, f.delta_R, sizeof(o.dR)); memcpy(o.dv, f.delta_v, sizeof(o.dv)); memcpy(o.dp, f.delta_p, sizeof(o.dp));
    memcpy(o.J_dR_bg, f.J_dR_bg, 72); memcpy(o.J_dv_ba, f.J_dv_ba, 72); memcpy(o.J_dv_bg, f.J_dv_bg, 72);
    memcpy(o.J_dp_ba, f.J_dp_ba, 72); memcpy(o.J_dp_bg, f.J_dp_bg, 72);
    if (!imu_sqrt_information(f.cov, o.W)) return false;
    o.sa = 1.0 / sqrt(f.dt * f.bacc_noise * f.bacc_noise);
    o.sg = 1.0 / sqrt(f.dt * f.bgyr_noise * f.bgyr_noise);
    o.win = 0; o.pad = 0;
    return true;
}

int sadvio_ba_set_imu_factors(sadvio_ba_handle* h, int32_t w, int32_t n, const sadvio_imu_factor* fs) {
    if (!h) return SADVIO_E_INVALID_ARG;
    if (!h->uploaded) { h->err = "set_imu_factors before set_windows"; return SADVIO_E_STATE; }
    if (w < 0 || w >= (int)h->plan.wins.size() || n < 0 || (n > 0 && !fs)) { h->err = "set_imu_factors: bad argument"; return SADVIO_E_INVALID_ARG; }
    const WinDev& d = h->plan.wins[w].d;
    if (n > 0 && !d.has_imu) { h->err = "set_imu_factors: the window was uploaded with has_imu = 0"; return SADVIO_E_INVALID_ARG; }
    HIP_TRY(hipSetDevice(h->device));
    auto& v = h->imus_per_win[w];
    v.clear();
    for (int k = 0; k < n; k++) {
        const sadvio_imu_factor& f = fs[k];
        if (f.kf_i < 0 || f.kf_i >= d.n_kf || f.kf_j < 0 || f.kf_j >= d.n_kf || f.kf_i == f.kf_j || !(f.dt > 0)) {
            h->err = "set_imu_factors: key-frame index / dt out of range"; return SADVIO_E_INVALID_ARG;
        }
        ImuDev o{};
        o.kf_i = d.kf_base + f.kf_i; o.kf_j = d.kf_base + f.kf_j; o.dt = f.dt;
        memcpy(o.dR, f.delta_R, sizeof(o.dR)); memcpy(o.dv, f.delta_v, sizeof(o.dv)); memcpy(o.dp, f.delta_p, sizeof(o.dp));
        memcpy(o.J_dR_bg, f.J_dR_bg, 72); memcpy(o.J_dv_ba, f.J_dv_ba, 72); memcpy(o.J_dv_bg, f.J_dv_bg, 72);
        memcpy(o.J_dp_ba, f.J_dp_ba, 72); memcpy(o.J_dp_bg, f.J_dp_bg, 72);
        if (!imu_sqrt_information(f.cov, o.W)) { h->err = "set_imu_factors: covariance is not positive definite"; return SADVIO_E_INVALID_ARG; }
        o.sa = 1.0 / sqrt(f.dt * f.bacc_noise * f.bacc_noise);
        o.sg = 1.0 / sqrt(f.dt * f.bgyr_noise * f.bgyr_noise);
        v.push_back(o);
    }
    if (h->defer) { h->pending = true; return SADVIO_OK; }
    h->up.reset();
    return upload_priors(h);
}

int sadvio_ba_set_dense_prior(sadvio_ba_handle* h, int32_t w, int32_t n_full, int32_t n, const double* J, const double* r0,
                              int32_t kf_keep, int32_t kf_col, int32_t n_keep, const int32_t* lmk_index, const int32_t* lmk_col) {
    if (!h) return SADVIO_E_INVALID_ARG;
    if (!h->uploaded) { h->err = "set_dense_prior before set_windows"; return SADVIO_E_STATE; }
    if (w < 0 || w >= (int)h->plan.wins.size() || (n_full < 0 && n_full != SADVIO_PRIOR_RESIDENT) || (n < 0 && n_full != SADVIO_PRIOR_RESIDENT) || n_keep < 0) { h->err = "set_dense_prior: bad argument"; return SADVIO_E_INVALID_ARG; }
    HIP_TRY(hipSetDevice(h->device));
    // a window sharded over several GPUs carries a dense prior too (round 5): every rank holds the prior and its variables — the kept
    // frame is replicated anyway, the kept landmarks are in every rank's window (with their observations on rank 0 only:
    // sadvio_amd/sharding.py) — rank 0 adds J^T J / J^T r to the all-reduced system, every rank evaluates the cost with the same bits
    const WinDev& d = h->plan.wins[w].d;
    DensePriorHost D;
    const bool resident = n_full == SADVIO_PRIOR_RESIDENT;
    if (resident) {
        if (J || r0) { h->err = "set_dense_prior: SADVIO_PRIOR_RESIDENT takes J = r0 = NULL"; return SADVIO_E_INVALID_ARG; }
        if (!h->prior.valid) { h->err = "set_dense_prior: SADVIO_PRIOR_RESIDENT but the handle holds no prior"; return SADVIO_E_STATE; }
        if (h->world > 1) { h->err = "set_dense_prior: not supported on a window sharded over several GPUs"; return SADVIO_E_INVALID_ARG; }
        n_full = h->prior.n_full; n = h->prior.n;
    }
    if (n_full > 0) {
        if ((!resident && (!J || !r0)) || n <= 0 || (n_keep > 0 && (!lmk_index || !lmk_col))) { h->err = "set_dense_prior: missing array"; return SADVIO_E_INVALID_ARG; }
        if (kf_keep >= d.n_kf || (kf_keep >= 0 && (kf_col < 0 || kf_col + 15 > n))) { h->err = "set_dense_prior: kept key-frame block out of range"; return SADVIO_E_INVALID_ARG; }
        std::vector<char> used(n, 0);
        if (kf_keep >= 0) for (int q = 0; q < 15; q++) used[kf_col + q] = 1;
        for (int i = 0; i < n_keep; i++) {
            if (lmk_col[i] < 0) continue;
            if (lmk_index[i] < 0 || lmk_index[i] >= d.n_lmk || lmk_col[i] + 3 > n) { h->err = "set_dense_prior: kept landmark out of range"; return SADVIO_E_INVALID_ARG; }
            if (lmk_is_refused_long(h, w, lmk_index[i])) {   // (SADVIO_CFG_LONG_TRACK_PRIORS: kept like any landmark, layout_reduced_plan)
                h->err = "set_dense_prior: landmark " + std::to_string(lmk_index[i]) + " is a long track (more than 64 observations): it cannot be kept in the reduced system";
                return SADVIO_E_INVALID_ARG;
            }
            for (int a = 0; a < 3; a++) {
                if (used[lmk_col[i] + a]) { h->err = "set_dense_prior: overlapping column blocks"; return SADVIO_E_INVALID_ARG; }
                used[lmk_col[i] + a] = 1;
            }
            // sharded window (sadvio_ba.h): the kept landmarks' observations live on rank 0 ONLY — every rank adds its kept rows to the
            // all-reduced system, so observations present on two ranks would be counted twice without any error
            if (h->world > 1 && h->rank != 0) {
                const int32_t* op = h->src[w].v.lmk_obs_ptr;
                if (op && op[lmk_index[i] + 1] != op[lmk_index[i]]) {
                    h->err = "set_dense_prior: on a sharded window the kept landmarks carry their observations on rank 0 only (landmark " + std::to_string(lmk_index[i]) + " has some on rank " + std::to_string(h->rank) + ")";
                    return SADVIO_E_INVALID_ARG;
                }
            }
        }
        D.n_full = n_full; D.n = n; D.kf_keep = kf_keep; D.kf_col = kf_col;
        D.resident = resident; D.serial = h->prior.serial;
        if (!resident) { D.J.assign(J, J + (size_t)n_full * n); D.r0.assign(r0, r0 + n_full); }
        D.lmk_index.assign(lmk_index, lmk_index + n_keep); D.lmk_col.assign(lmk_col, lmk_col + n_keep);
    }
    h->dprior_per_win[w] = std::move(D);
    if (h->defer) { h->pending = true; return SADVIO_OK; }
    if (!h->sparse_per_win[w].empty()) return layout_build(h);  // which sparse factors are eliminable may change
    h->up.reset();
    int rc = layout_reduced(h);
    if (rc != SADVIO_OK) return rc;
    if (h->defer) { h->pending = true; return SADVIO_OK; }
    return upload_priors(h);
}

int sadvio_ba_set_sparse_priors(sadvio_ba_handle* h, int32_t w, int32_t n, const sadvio_sparse_prior* f) {
    if (!h) return SADVIO_E_INVALID_ARG;
    if (!h->uploaded) { h->err = "set_sparse_priors before set_windows"; return SADVIO_E_STATE; }
    if (w < 0 || w >= (int)h->plan.wins.size() || n < 0 || (n > 0 && !f)) { h->err = "set_sparse_priors: bad argument"; return SADVIO_E_INVALID_ARG; }
    HIP_TRY(hipSetDevice(h->device));
    const WinDev& d = h->plan.wins[w].d;
    for (int i = 0; i < n; i++) {
        const sadvio_sparse_prior& s = f[i];
        // A window sharded over several GPUs carries the SPARSIFIED VIO prior (what sparsifyVIO produces): IMUPriordx is a
        // pose-only factor every rank evaluates identically after the all-reduce, a PoseToLandmarkFactor on a free landmark
        // rides the elimination of the rank that owns the landmark. Factors that hold landmarks in the reduced system
        // (Landmark3DPrior, landmark chains, relative poses of other layouts) would need those landmarks on every rank.
        if (h->world > 1 && !(s.type == SADVIO_SPARSE_IMU_PRIOR || (s.type == SADVIO_SPARSE_POSE_TO_LMK && s.lmk0 >= 0 && s.lmk0 < d.n_lmk &&
                                                                     !(h->src[w].v.lmk_const && h->src[w].v.lmk_const[s.lmk0])))) {
            h->err = "set_sparse_priors: a window sharded over several GPUs takes IMU-prior and pose-to-landmark factors (on free landmarks of this rank) only";
            return SADVIO_E_INVALID_ARG;
        }
        const bool rel = s.type == SADVIO_SPARSE_RELATIVE_POSE;
        if (rel && (s.kf_b < 0 || s.kf_b >= d.n_kf || s.kf_b == s.kf || d.dpf != 6)) {
            h->err = "set_sparse_priors: relative-pose factor " + std::to_string(i) + " has a bad key-frame (or the window carries IMU states)";
            return SADVIO_E_INVALID_ARG;
        }
        const bool need_kf = s.type == SADVIO_SPARSE_IMU_PRIOR || s.type == SADVIO_SPARSE_POSE_TO_LMK || rel;
        const bool need_l0 = s.type != SADVIO_SPARSE_IMU_PRIOR && !rel, need_l1 = s.type == SADVIO_SPARSE_LMK_TO_LMK;
        if (s.type < 0 || s.type > 4 || (need_kf && (s.kf < 0 || s.kf >= d.n_kf)) || (need_l0 && (s.lmk0 < 0 || s.lmk0 >= d.n_lmk)) ||
            (need_l1 && (s.lmk1 < 0 || s.lmk1 >= d.n_lmk || s.lmk1 == s.lmk0))) {
            h->err = "set_sparse_priors: factor " + std::to_string(i) + " has a bad type or index";
            return SADVIO_E_INVALID_ARG;
        }
    }
    // long tracks (long_kernels.h) carry real observations only; they are held in the reduced system on a handle created with
    // SADVIO_CFG_LONG_TRACK_PRIORS only (there a pose-to-landmark factor on one holds it as well: layout_views)
    if (h->env.long_min > 0 && h->world == 1 && !h->coll_fn) {
        const std::vector<int32_t>& op = h->src[w].lmk_obs_ptr;
        std::vector<int> pseudo(std::max(d.n_lmk, 1), 0);
        for (int i = 0; i < n; i++) {
            const sadvio_sparse_prior& s = f[i];
            if (s.type == SADVIO_SPARSE_IMU_PRIOR || s.type == SADVIO_SPARSE_RELATIVE_POSE) continue;
            if (lmk_is_refused_long(h, w, s.lmk0) || (s.type == SADVIO_SPARSE_LMK_TO_LMK && lmk_is_refused_long(h, w, s.lmk1))) {
                h->err = "set_sparse_priors: factor " + std::to_string(i) + " touches a long track (a landmark with more than 64 observations)";
                return SADVIO_E_INVALID_ARG;
            }
            if (s.type == SADVIO_SPARSE_POSE_TO_LMK && !lmk_is_long(h, w, s.lmk0) && (int)op.size() > s.lmk0 + 1 && op[s.lmk0 + 1] - op[s.lmk0] + (pseudo[s.lmk0] += 2) > MAX_LMK_OBS) {
                h->err = "set_sparse_priors: factor " + std::to_string(i) + " would make its landmark a long track (more than 64 observations with the factors' pseudo-observations)";
                return SADVIO_E_INVALID_ARG;
            }
        }
    }
    h->sparse_per_win[w].assign(f, f + n);
    if (h->defer) { h->pending = true; return SADVIO_OK; }
    return layout_build(h);  // eliminable pose-to-landmark factors become pseudo-observations: the tiles change
}

}  // extern "C"

#include "marg_driver.h"   // below make_imu_dev: marg_layout builds frame0's IMU factor with it

extern "C" {

int sadvio_ba_marginalize(sadvio_ba_handle* h, int32_t w, const sadvio_marg_request* rq, sadvio_marg_result* res, int32_t* lmk_col_out,
                          double* J_out, double* r0_out) {
    if (!h) return SADVIO_E_INVALID_ARG;
    if (!h->uploaded) { h->err = "marginalize before set_windows"; return SADVIO_E_STATE; }
    if (h->defer) { h->err = "marginalize between begin_update and commit_update"; return SADVIO_E_STATE; }
    if (!rq || w < 0 || w >= (int)h->plan.wins.size()) { h->err = "marginalize: bad argument"; return SADVIO_E_INVALID_ARG; }
    if (h->world > 1) { h->err = "marginalize: the window is sharded over several GPUs (each rank holds a landmark partition only)"; return SADVIO_E_INVALID_ARG; }
    // (SADVIO_CFG_LONG_TRACK_PRIORS: served. marg_layout lists one item per observation from lmk_ob / lmk_oe / obs_perm, which hold a long
    // track's observations like any others, and k_marg_obs takes an item by its device index: nothing there walks a lane group)
    if (!h->env.long_priors)
        if (int rc = refuse_long(h, w, "marginalize")) return rc;
    return marginalize(h, w, rq, res, lmk_col_out, J_out, r0_out);
}

int sadvio_ba_marg_stats(sadvio_ba_handle* h, int32_t* calls, int32_t* unpivoted, int32_t* fell_back) {
    if (!h) return SADVIO_E_INVALID_ARG;
    if (calls) *calls = h->marg_stats[0];
    if (unpivoted) *unpivoted = h->marg_stats[1];
    if (fell_back) *fell_back = h->marg_stats[2];
    return SADVIO_OK;
}

int sadvio_ba_get_prior(sadvio_ba_handle* h, sadvio_prior_info* info, double* J, double* r0) {
    if (!h) return SADVIO_E_INVALID_ARG;
    const PriorState& PR = h->prior;
    if (info) { info->valid = PR.valid ? 1 : 0; info->n_full = PR.valid ? PR.n_full : 0; info->n = PR.valid ? PR.n : 0; info->form = PR.form; }
    if (!PR.valid) { if (J || r0) { h->err = "get_prior: the handle holds no prior"; return SADVIO_E_STATE; } return SADVIO_OK; }
    HIP_TRY(hipSetDevice(h->device));
    if (J) HIP_TRY(hipMemcpyAsync(J, PR.J.p, sizeof(double) * (size_t)PR.n_full * PR.n, hipMemcpyDeviceToHost, h->stream));
    if (r0) HIP_TRY(hipMemcpyAsync(r0, PR.r0.p, sizeof(double) * PR.n_full, hipMemcpyDeviceToHost, h->stream));
    HIP_TRY(hipStreamSynchronize(h->stream));
    return SADVIO_OK;
}

int sadvio_ba_set_prior(sadvio_ba_handle* h, int32_t n_full, int32_t n, int32_t form, const double* J, const double* r0) {
    if (!h) return SADVIO_E_INVALID_ARG;
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

int sadvio_ba_marginalize_relative(sadvio_ba_handle* h, int32_t w, int32_t kf_a, int32_t kf_b, int32_t eig_cut_mode, double* inf36, double* Ak144) {
    if (!h || !inf36) return SADVIO_E_INVALID_ARG;
    if (!h->uploaded) { h->err = "marginalize_relative before set_windows"; return SADVIO_E_STATE; }
    if (h->defer) { h->err = "marginalize_relative between begin_update and commit_update"; return SADVIO_E_STATE; }
    if (w < 0 || w >= (int)h->plan.wins.size()) { h->err = "marginalize_relative: window out of range"; return SADVIO_E_INVALID_ARG; }
    if (eig_cut_mode != SADVIO_EIG_CUT_REFERENCE && eig_cut_mode != SADVIO_EIG_CUT_NOISE_FLOOR) { h->err = "marginalize_relative: bad eig_cut_mode"; return SADVIO_E_INVALID_ARG; }
    if (h->world > 1) { h->err = "marginalize_relative: the window is sharded over several GPUs (each rank holds a landmark partition only)"; return SADVIO_E_INVALID_ARG; }
    const WinDev& d = h->plan.wins[w].d;
    if (kf_a < 0 || kf_a >= d.n_kf || kf_b < 0 || kf_b >= d.n_kf || kf_a == kf_b) { h->err = "marginalize_relative: bad key-frame index"; return SADVIO_E_INVALID_ARG; }
    if (!h->env.long_batch)   // (SADVIO_CFG_LONG_TRACK_BATCH: served; a long track's observations are found by bisection, rel_runs.h)
        if (int rc = refuse_long(h, w, "marginalize_relative")) return rc;
    if (d.has_imu) { h->err = "marginalize_relative: frames with IMU states are not supported (the reference's own column layout for them is inconsistent, BundleAdjustmentCERESAnalytic.cpp:705-737)"; return SADVIO_E_INVALID_ARG; }
    return marginalize_relative(h, w, kf_a, kf_b, eig_cut_mode, inf36, Ak144);
}

int sadvio_ba_sparsify(sadvio_ba_handle* h, int32_t w, int32_t vio, int32_t nf, int32_t n, const double* J, int32_t kf_keep,
                       int32_t kf_col, int32_t n_keep, const int32_t* lmk_index, const int32_t* lmk_col, int32_t* n_out,
                       sadvio_sparse_prior* out) {
    if (!h) return SADVIO_E_INVALID_ARG;
    if (n_out) *n_out = 0;
    if (!h->uploaded) { h->err = "sparsify before set_windows"; return SADVIO_E_STATE; }
    if (h->defer) { h->err = "sparsify between begin_update and commit_update"; return SADVIO_E_STATE; }
    if (w < 0 || w >= (int)h->plan.wins.size() || !n_out || !out || n_keep < 0 || (n_keep > 0 && (!lmk_index || !lmk_col))) { h->err = "sparsify: bad argument"; return SADVIO_E_INVALID_ARG; }
    if (h->world > 1) { h->err = "sparsify: the window is sharded over several GPUs (linearisation values of a landmark partition only)"; return SADVIO_E_INVALID_ARG; }
    for (int i = 0; i < n_keep; i++)
        if (lmk_is_refused_long(h, w, lmk_index[i])) { h->err = "sparsify: landmark " + std::to_string(lmk_index[i]) + " is a long track (more than 64 observations)"; return SADVIO_E_INVALID_ARG; }
    return sparsify(h, w, vio, nf, n, J, kf_keep, kf_col, n_keep, lmk_index, lmk_col, n_out, out);
}

int sadvio_ba_set_collective(sadvio_ba_handle* h, int32_t rank, int32_t world, sadvio_allreduce_fn fn, void* ctx) {
    if (!h) return SADVIO_E_INVALID_ARG;
    if (world < 1 || rank < 0 || rank >= world || (world > 1 && !fn)) { h->err = "set_collective: bad rank / world / callback"; return SADVIO_E_INVALID_ARG; }
    if (h->uploaded) { h->err = "set_collective must precede set_windows (the buffer layout depends on the world size)"; return SADVIO_E_STATE; }
    h->rank = rank; h->world = world; h->coll_fn = fn; h->coll_ctx = ctx;
    return SADVIO_OK;
}

namespace {
static std::string load_rccl(RcclLib& R) {
    if (R.lib) return "";
    R.lib = dlopen("librccl.so.1", RTLD_NOW | RTLD_LOCAL);
    if (!R.lib) R.lib = dlopen("librccl.so", RTLD_NOW | RTLD_LOCAL);
    if (!R.lib) return std::string("dlopen librccl: ") + dlerror();
    R.get_id = (int (*)(NcclId*))dlsym(R.lib, "ncclGetUniqueId");
    R.init_rank = (int (*)(void**, int, NcclId, int))dlsym(R.lib, "ncclCommInitRank");
    R.all_reduce = (int (*)(const void*, void*, size_t, int, int, void*, hipStream_t))dlsym(R.lib, "ncclAllReduce");
    R.destroy = (int (*)(void*))dlsym(R.lib, "ncclCommDestroy");
    R.err_string = (const char* (*)(int))dlsym(R.lib, "ncclGetErrorString");
    R.comm_count = (int (*)(void*, int*))dlsym(R.lib, "ncclCommCount");
    R.comm_user_rank = (int (*)(void*, int*))dlsym(R.lib, "ncclCommUserRank");
    R.comm_cu_device = (int (*)(void*, int*))dlsym(R.lib, "ncclCommCuDevice");
    if (!R.get_id || !R.init_rank || !R.all_reduce || !R.destroy) return "missing RCCL symbol";
    return "";
}
int rccl_allreduce(void* ctx, double* buf, int64_t count, void* stream) {
    sadvio_ba_handle* h = (sadvio_ba_handle*)ctx;
    // ncclDouble = 8, ncclSum = 0; in place
    return h->rccl.all_reduce(buf, buf, (size_t)count, 8, 0, h->rccl.comm, (hipStream_t)stream);
}
}  // namespace

int sadvio_ba_rccl_unique_id(void* id128) {
    if (!id128) return SADVIO_E_INVALID_ARG;
    RcclLib R;
    const std::string e = load_rccl(R);
    if (!e.empty()) return SADVIO_E_RCCL;
    NcclId id;
    if (R.get_id(&id) != 0) return SADVIO_E_RCCL;
    memcpy(id128, &id, sizeof(id));
    return SADVIO_OK;  // the library stays loaded (process lifetime)
}

int sadvio_ba_comm_init_rccl(sadvio_ba_handle* h, int32_t rank, int32_t world, const void* id128) {
    if (!h) return SADVIO_E_INVALID_ARG;
    if (!id128 || world < 1 || rank < 0 || rank >= world) { h->err = "comm_init_rccl: bad argument"; return SADVIO_E_INVALID_ARG; }
    if (h->uploaded) { h->err = "comm_init_rccl must precede set_windows"; return SADVIO_E_STATE; }
    HIP_TRY(hipSetDevice(h->device));
    const std::string e = load_rccl(h->rccl);
    if (!e.empty()) { h->err = "comm_init_rccl: " + e; return SADVIO_E_RCCL; }
    NcclId id;
    memcpy(&id, id128, sizeof(id));
    const int rc = h->rccl.init_rank(&h->rccl.comm, world, id, rank);
    if (rc != 0) {
        h->err = std::string("comm_init_rccl: ncclCommInitRank: ") + (h->rccl.err_string ? h->rccl.err_string(rc) : "error");
        h->rccl.comm = nullptr;
        return SADVIO_E_RCCL;
    }
    h->rank = rank; h->world = world; h->coll_fn = rccl_allreduce; h->coll_ctx = h;
    return SADVIO_OK;
}

int sadvio_ba_comm_info(sadvio_ba_handle* h, int32_t* nranks, int32_t* rank, int32_t* device, int32_t* is_rccl) {
    if (!h) return SADVIO_E_INVALID_ARG;
    int n = h->world, r = h->rank, d = h->device;
    const bool rccl = h->rccl.comm != nullptr;
    if (rccl) {   // what the COMMUNICATOR says, not what it was asked for
        if (!h->rccl.comm_count || !h->rccl.comm_user_rank || h->rccl.comm_count(h->rccl.comm, &n) != 0 || h->rccl.comm_user_rank(h->rccl.comm, &r) != 0) {
            h->err = "comm_info: ncclCommCount / ncclCommUserRank failed"; return SADVIO_E_RCCL;
        }
        if (h->rccl.comm_cu_device) (void)h->rccl.comm_cu_device(h->rccl.comm, &d);
    }
    if (nranks) *nranks = n;
    if (rank) *rank = r;
    if (device) *device = d;
    if (is_rccl) *is_rccl = rccl ? 1 : 0;
    return SADVIO_OK;
}

namespace {
// The caller's options as the kernels take them; null: the defaults
int convert_options(sadvio_ba_handle* h, const sadvio_solve_options* opts, SolveOpts& o) {
    sadvio_solve_options defo;
    if (!opts) { sadvio_ba_default_options(&defo); opts = &defo; }
    if (opts->max_num_iterations < 0 || opts->max_num_iterations > 1000) { h->err = "solve: max_num_iterations out of range"; return SADVIO_E_INVALID_ARG; }
    memset(&o, 0, sizeof(o));   // it travels in DevPtrs, whose bytes are part of the graph key
    o.max_num_iterations = opts->max_num_iterations; o.jacobi_scaling = opts->jacobi_scaling;
    o.max_num_consecutive_invalid_steps = opts->max_num_consecutive_invalid_steps;
    o.function_tolerance = opts->function_tolerance; o.gradient_tolerance = opts->gradient_tolerance;
    o.parameter_tolerance = opts->parameter_tolerance; o.initial_radius = opts->initial_trust_region_radius;
    o.max_radius = opts->max_trust_region_radius; o.min_radius = opts->min_trust_region_radius;
    o.min_lm_diagonal = opts->min_lm_diagonal; o.max_lm_diagonal = opts->max_lm_diagonal;
    o.min_relative_decrease = opts->min_relative_decrease;
    o.huber_a = opts->huber_a;
    // wall_clock64: 100 MHz. Not applied to a window sharded over several GPUs: the ranks' clocks would disagree on the slot
    o.max_time_ticks = (opts->max_solver_time_in_seconds > 0.0 && h->world == 1) ? opts->max_solver_time_in_seconds * 1e8 : 0.0;
    if (!(o.huber_a >= 0.0)) { h->err = "solve: huber_a must be >= 0"; return SADVIO_E_INVALID_ARG; }
    return SADVIO_OK;
}
}  // namespace

int sadvio_ba_solve(sadvio_ba_handle* h, const sadvio_solve_options* opts, sadvio_solve_summary* summaries) {
    if (!h) return SADVIO_E_INVALID_ARG;
    if (!h->uploaded) { h->err = "solve before set_windows"; return SADVIO_E_STATE; }
    if (h->defer) { h->err = "solve between begin_update and commit_update"; return SADVIO_E_STATE; }
    // 1. options
    SolveOpts o;
    if (int rc = convert_options(h, opts, o)) return rc;
    HIP_TRY(hipSetDevice(h->device));
    // 2. plan: everything the launch sequence reads
    SolvePlan plan;
    std::vector<BigPlan> big;
    if (int rc = plan_solve(h, o, plan, big)) return rc;
    // 3. launch, as one graph where the handle asks for it
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
    // 4. wait, collect the timers
    HIP_TRY(hipStreamSynchronize(h->stream));
    if (h->cfg.profile_kernels) collect_timers(h);
    // 5. diagnostics
    if (h->env.debug & 4096) print_debug_stamps(h, plan.P.n_tiles);
    // 6. summaries
    const int n_win = plan.P.n_win;
    h->fin.assign(h->h_final, h->h_final + n_win);
    h->deltas_cached = false;
    h->last_slots = plan.slots;
    h->cov_huber_a = o.huber_a; h->cov_use_lm = plan.use_lm;
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

int sadvio_ba_get_deltas(sadvio_ba_handle* h, int32_t w, double* pose, double* lmk, double* dv, double* dba, double* dbg) {
    if (!h) return SADVIO_E_INVALID_ARG;
    if (!h->solved) { h->err = "get_deltas before solve"; return SADVIO_E_STATE; }
    if (w < 0 || w >= (int)h->plan.wins.size()) { h->err = "get_deltas: window out of range"; return SADVIO_E_INVALID_ARG; }
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

int sadvio_ba_get_trace(sadvio_ba_handle* h, int32_t w, int32_t cap_rows, double* rows8, int32_t* n_rows) {
    if (!h) return SADVIO_E_INVALID_ARG;
    if (!h->solved) { h->err = "get_trace before solve"; return SADVIO_E_STATE; }
    if (w < 0 || w >= (int)h->plan.wins.size() || cap_rows < 0 || (cap_rows > 0 && !rows8)) { h->err = "get_trace: bad argument"; return SADVIO_E_INVALID_ARG; }
    HIP_TRY(hipSetDevice(h->device));
    const int stride = h->last_slots + 2;
    const int n = std::min(h->fin[w].s.iter + 1, stride);
    if (n_rows) *n_rows = n;
    const int m = std::min(n, cap_rows);
    if (m > 0) HIP_TRY(hipMemcpy(rows8, h->d_trace.p + (size_t)w * stride * 8, sizeof(double) * 8 * (size_t)m, hipMemcpyDeviceToHost));
    return SADVIO_OK;
}

int sadvio_ba_get_ids(sadvio_ba_handle* h, int32_t w, int64_t* kf_id, int64_t* lmk_id) {
    if (!h) return SADVIO_E_INVALID_ARG;
    if (w < 0 || w >= (int)h->plan.wins.size()) { h->err = "get_ids: window out of range"; return SADVIO_E_INVALID_ARG; }
    if (kf_id) memcpy(kf_id, h->plan.wins[w].kf_id.data(), sizeof(int64_t) * h->plan.wins[w].kf_id.size());
    if (lmk_id) memcpy(lmk_id, h->plan.wins[w].lmk_id.data(), sizeof(int64_t) * h->plan.wins[w].lmk_id.size());
    return SADVIO_OK;
}

int sadvio_ba_linearize(sadvio_ba_handle* h, int32_t w, const double* pose_delta6, const double* lmk_delta3, double* r2,
                        double* Jp12, double* Jl6) {
    if (!h) return SADVIO_E_INVALID_ARG;
    if (!h->uploaded) { h->err = "linearize before set_windows"; return SADVIO_E_STATE; }
    if (h->defer) { h->err = "linearize between begin_update and commit_update"; return SADVIO_E_STATE; }
    if (w < 0 || w >= (int)h->plan.wins.size()) { h->err = "linearize: window out of range"; return SADVIO_E_INVALID_ARG; }
    HIP_TRY(hipSetDevice(h->device));
    const WinDev& d = h->plan.wins[w].d;
    HIP_TRY(hipMemsetAsync(h->d_xp.p, 0, sizeof(double) * h->d_xp.n, h->stream));
    HIP_TRY(hipMemsetAsync(h->d_xl.p, 0, sizeof(double) * h->d_xl.n, h->stream));
    if (pose_delta6) HIP_TRY(hipMemcpyAsync(h->d_xp.p + 6 * (size_t)d.kf_base, pose_delta6, sizeof(double) * 6 * d.n_kf, hipMemcpyHostToDevice, h->stream));
    if (lmk_delta3 && d.n_lmk) HIP_TRY(hipMemcpyAsync(h->d_xl.p + 3 * (size_t)d.lmk_base, lmk_delta3, sizeof(double) * 3 * d.n_lmk, hipMemcpyHostToDevice, h->stream));
    if (d.n_obs == 0) { HIP_TRY(hipStreamSynchronize(h->stream)); return SADVIO_OK; }
    HIP_TRY(h->d_probe.alloc(20 * (size_t)d.n_obs));
    SolveOpts o{};
    DevPtrs P = make_ptrs(h, o, 1);
    double* pr = h->d_probe.p; double* pj = pr + 2 * (size_t)d.n_obs; double* pl = pj + 12 * (size_t)d.n_obs;
    int blocks = (d.n_obs + 255) / 256;
    if (h->plan.factor_type == SADVIO_FACTOR_PIXEL) hipLaunchKernelGGL(k_linearize_probe<0>, dim3(blocks), dim3(256), 0, h->stream, P, w, pr, pj, pl);
    else hipLaunchKernelGGL(k_linearize_probe<1>, dim3(blocks), dim3(256), 0, h->stream, P, w, pr, pj, pl);
    HIP_TRY(hipGetLastError());
    std::vector<double> hb(20 * (size_t)d.n_obs);
    HIP_TRY(hipMemcpyAsync(hb.data(), pr, sizeof(double) * 20 * (size_t)d.n_obs, hipMemcpyDeviceToHost, h->stream));
    HIP_TRY(hipStreamSynchronize(h->stream));
    for (int a = 0; a < d.n_obs; a++) {
        const int src = h->plan.obs_perm[d.obs_base + a];  // caller's index of the observation stored at position a
        if (src < 0) continue;                          // pseudo-observation
        if (r2) memcpy(r2 + 2 * (size_t)src, &hb[2 * (size_t)a], 16);
        if (Jp12) memcpy(Jp12 + 12 * (size_t)src, &hb[2 * (size_t)d.n_obs + 12 * (size_t)a], 96);
        if (Jl6) memcpy(Jl6 + 6 * (size_t)src, &hb[14 * (size_t)d.n_obs + 6 * (size_t)a], 48);
    }
    h->solved = false;
    return SADVIO_OK;
}

int sadvio_ba_vi_init(sadvio_ba_handle* h, const sadvio_viinit_problem* pb, const sadvio_solve_options* opts, sadvio_solve_summary* sum,
                      sadvio_viinit_result* res, double* dv3) {
    if (!h) return SADVIO_E_INVALID_ARG;
    if (!pb || !opts || pb->n_frames < 0 || pb->n_factors < 0 || (pb->n_frames > 0 && (!pb->T_f_w || !pb->vel)) || (pb->n_factors > 0 && !pb->factors)) {
        h->err = "vi_init: bad argument"; return SADVIO_E_INVALID_ARG;
    }
    if (pb->n_frames > VIINIT_MAX_FRAMES) { h->err = "vi_init: more than 48 frames"; return SADVIO_E_INVALID_ARG; }
    if (pb->optim_bias && !(pb->sigma_dba > 0.0 && pb->sigma_dbg > 0.0)) { h->err = "vi_init: bias prior sigmas must be positive"; return SADVIO_E_INVALID_ARG; }
    HIP_TRY(hipSetDevice(h->device));
    const int n = pb->n_frames, nf = pb->n_factors;
    // program layout: r_wi | velocity deltas of the frames a factor touches (frame order) | dba dbg | lambda
    std::vector<int> vcol(std::max(n, 1), -1);
    std::vector<ImuDev> fd(std::max(nf, 1));
    for (int k = 0; k < nf; k++) {
        const sadvio_imu_factor& f = pb->factors[k];
        if (f.kf_i < 0 || f.kf_i >= n || f.kf_j < 0 || f.kf_j >= n || f.kf_i == f.kf_j) { h->err = "vi_init: factor frame index out of range"; return SADVIO_E_INVALID_ARG; }
        if (!make_imu_dev(f, 0, fd[k])) { h->err = "vi_init: IMU covariance is not positive definite"; return SADVIO_E_INVALID_ARG; }
        vcol[f.kf_i] = vcol[f.kf_j] = 0;
    }
    int D = 2;
    for (int i = 0; i < n; i++) if (vcol[i] == 0) { vcol[i] = D; D += 3; }
    ViInitDev P{};
    P.n_frames = n; P.n_factors = nf; P.optim_bias = pb->optim_bias ? 1 : 0;
    P.c_ba = P.c_bg = P.c_l = -1;
    if (pb->optim_bias) { P.c_ba = D; P.c_bg = D + 3; D += 6; P.isig_ba = 1.0 / pb->sigma_dba; P.isig_bg = 1.0 / pb->sigma_dbg; }
    if (pb->optim_scale) { P.c_l = D; D += 1; }
    P.D = D;
    std::vector<double> out((size_t)D + 8, 0.0);
    sadvio_solve_summary S{};
    if (nf == 0) S.termination = SADVIO_TERM_GRADIENT_TOL;   // empty program: Ceres returns at once
    else {
        P.o.max_num_iterations = opts->max_num_iterations; P.o.jacobi_scaling = opts->jacobi_scaling;
        P.o.max_num_consecutive_invalid_steps = opts->max_num_consecutive_invalid_steps;
        P.o.function_tolerance = opts->function_tolerance; P.o.gradient_tolerance = opts->gradient_tolerance;
        P.o.parameter_tolerance = opts->parameter_tolerance; P.o.initial_radius = opts->initial_trust_region_radius;
        P.o.max_radius = opts->max_trust_region_radius; P.o.min_radius = opts->min_trust_region_radius;
        P.o.min_lm_diagonal = opts->min_lm_diagonal; P.o.max_lm_diagonal = opts->max_lm_diagonal; P.o.min_relative_decrease = opts->min_relative_decrease;
        // one allocation: header | T | vel | out | scratch | factors | vcol
        const size_t n_d = 12 * (size_t)n + 3 * (size_t)n + out.size() + 2 * (size_t)nf * VIINIT_FJ;
        const size_t bytes = sizeof(ViInitDev) + 8 * n_d + sizeof(ImuDev) * (size_t)nf + sizeof(int) * (size_t)n + 64;
        DevBuf<char> buf;
        HIP_TRY(buf.alloc(bytes));
        char* base = buf.p;
        double* dT = (double*)(base + ((sizeof(ViInitDev) + 15) & ~(size_t)15));
        double* dvel = dT + 12 * (size_t)n; double* dout = dvel + 3 * (size_t)n; double* dscr = dout + out.size();
        ImuDev* df = (ImuDev*)(dscr + 2 * (size_t)nf * VIINIT_FJ);
        int* dvc = (int*)(df + nf);
        P.T = dT; P.vel = dvel; P.out = dout; P.scratch = dscr; P.f = df; P.vcol = dvc;
        HIP_TRY(hipMemcpyAsync(base, &P, sizeof(P), hipMemcpyHostToDevice, h->stream));
        HIP_TRY(hipMemcpyAsync(dT, pb->T_f_w, 96 * (size_t)n, hipMemcpyHostToDevice, h->stream));
        HIP_TRY(hipMemcpyAsync(dvel, pb->vel, 24 * (size_t)n, hipMemcpyHostToDevice, h->stream));
        HIP_TRY(hipMemcpyAsync(df, fd.data(), sizeof(ImuDev) * (size_t)nf, hipMemcpyHostToDevice, h->stream));
        HIP_TRY(hipMemcpyAsync(dvc, vcol.data(), sizeof(int) * (size_t)n, hipMemcpyHostToDevice, h->stream));
        const size_t lds = 8 * ((size_t)(D + 1) * (D + 2) / 2 + 6 * (size_t)D);
        HIP_TRY(hipFuncSetAttribute((const void*)k_viinit, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds));
        hipLaunchKernelGGL(k_viinit, dim3(1), dim3(VIINIT_THREADS), lds, h->stream, (const ViInitDev*)base);
        HIP_TRY(hipGetLastError());
        HIP_TRY(hipMemcpyAsync(out.data(), dout, 8 * out.size(), hipMemcpyDeviceToHost, h->stream));
        HIP_TRY(hipStreamSynchronize(h->stream));
        const double* s = out.data() + D;
        S.initial_cost = s[0]; S.final_cost = s[1]; S.final_radius = s[2]; S.iterations = (int)s[3]; S.termination = (int)s[4];
        S.num_successful_steps = (int)s[5]; S.num_unsuccessful_steps = (int)s[6];
    }
    if (sum) *sum = S;
    if (res) {
        memset(res, 0, sizeof(*res));
        res->r_wi[0] = out[0]; res->r_wi[1] = out[1];
        res->lambda = P.c_l >= 0 ? out[P.c_l] : 0.0;
        for (int a = 0; a < 3; a++) { res->dba[a] = P.c_ba >= 0 ? out[P.c_ba + a] : 0.0; res->dbg[a] = P.c_bg >= 0 ? out[P.c_bg + a] : 0.0; }
        host_exp_so3(res->r_wi[0], res->r_wi[1], res->R_w_i);
        res->scale = std::exp(res->lambda);
    }
    if (dv3)
        for (int i = 0; i < n; i++)
            for (int a = 0; a < 3; a++) dv3[3 * i + a] = vcol[i] >= 0 ? out[vcol[i] + a] : 0.0;
    return S.termination == SADVIO_TERM_FAILURE ? SADVIO_E_NOT_USABLE : SADVIO_OK;
}

// landmarkOptimizationNoFov (AngularAdjustmentCERESAnalytic.cpp:741-907): validation and the constant tables on the host,
// the whole LM solve and the gate in one launch of k_nofov (nofov_kernels.h)
int sadvio_ba_nofov_scale(sadvio_ba_handle* h, const sadvio_nofov_problem* pb, const sadvio_solve_options* opts, sadvio_solve_summary* sum,
                          sadvio_nofov_result* res, double* lmk_delta3, double* gate_norm, int32_t* inlier) {
    if (!h) return SADVIO_E_INVALID_ARG;
    if (!pb || !opts || pb->n_lmk < 0 || pb->n_obs < 0 || pb->n_frames < 1 || pb->n_cam < 1 || !pb->frame_T_f_w || !pb->cam_T_s_f ||
        !pb->T_cam0_cam0p || pb->cam0 < 0 || pb->cam0 >= pb->n_cam || pb->fix_scale < -1 || pb->fix_scale > 1 ||
        (pb->n_lmk > 0 && (!pb->lmk_p || !pb->scale_bearing || !pb->scale_cam || !pb->lmk_obs_ptr)) ||
        (pb->n_obs > 0 && (!pb->obs_frame || !pb->obs_cam || !pb->obs_bearing || !pb->lmk_obs_ptr))) {
        h->err = "nofov_scale: bad argument"; return SADVIO_E_INVALID_ARG;
    }
    const int n = pb->n_lmk, no = pb->n_obs, nfr = pb->n_frames, nc = pb->n_cam;
    if (n > NOFOV_MAX_LMK) { h->err = "nofov_scale: more than 65536 landmarks"; return SADVIO_E_INVALID_ARG; }
    if (n > 0) {
        if (pb->lmk_obs_ptr[0] != 0 || pb->lmk_obs_ptr[n] != no) { h->err = "nofov_scale: lmk_obs_ptr does not span n_obs"; return SADVIO_E_INVALID_ARG; }
        for (int l = 0; l < n; l++) {
            const int c = pb->lmk_obs_ptr[l + 1] - pb->lmk_obs_ptr[l];
            if (c < 0) { h->err = "nofov_scale: lmk_obs_ptr is not monotone"; return SADVIO_E_INVALID_ARG; }
            if (c > NOFOV_MAX_OBS_PER_LMK) { h->err = "nofov_scale: more than 16 angular factors on a landmark"; return SADVIO_E_INVALID_ARG; }
            if (pb->scale_cam[l] < 0 || pb->scale_cam[l] >= nc) { h->err = "nofov_scale: scale_cam out of range"; return SADVIO_E_INVALID_ARG; }
        }
    } else if (no != 0) { h->err = "nofov_scale: observations without landmarks"; return SADVIO_E_INVALID_ARG; }
    for (int o = 0; o < no; o++)
        if (pb->obs_frame[o] < 0 || pb->obs_frame[o] >= nfr || pb->obs_cam[o] < 0 || pb->obs_cam[o] >= nc) {
            h->err = "nofov_scale: observation index out of range"; return SADVIO_E_INVALID_ARG;
        }
    const double* Tm = pb->T_cam0_cam0p;
    int fixed = pb->fix_scale;
    if (fixed < 0) {   // :769-772: geometry::log_so3 (geometry.h:149-166) of the rotation, norm of the translation
        double c = (Tm[0] + Tm[4] + Tm[8]) / 2.0 - 0.5;
        c = std::min(std::max(c, -1.0), 1.0);
        const double ang = std::acos(c);
        const double d[3] = {Tm[7] - Tm[5], Tm[2] - Tm[6], Tm[3] - Tm[1]};
        const double f = (std::fabs(std::sin(ang)) < 1e-9 || ang < 1e-9) ? 0.5 : ang / (2.0 * std::sin(ang));
        const double rot = f * std::sqrt(d[0] * d[0] + d[1] * d[1] + d[2] * d[2]);
        const double tn = std::sqrt(Tm[9] * Tm[9] + Tm[10] * Tm[10] + Tm[11] * Tm[11]);
        fixed = (rot < 0.05 || tn < 0.01) ? 1 : 0;
    }
    if (n == 0 && fixed) { h->err = "nofov_scale: no landmark and a constant scale: nothing to solve"; return SADVIO_E_INVALID_ARG; }
    HIP_TRY(hipSetDevice(h->device));
    // constant tables: a zero-delta pose table per frame (angular_factor), A | b0 | v per camera (scale factor)
    std::vector<double> ftab(NOFOV_FTAB * (size_t)nfr), ctab(NOFOV_CTAB * (size_t)nc);
    const double I3[9] = {1, 0, 0, 0, 1, 0, 0, 0, 1};
    for (int k = 0; k < nfr; k++) {
        const double* T = pb->frame_T_f_w + 12 * (size_t)k;
        double* o = &ftab[NOFOV_FTAB * (size_t)k];
        memcpy(o, T, 96); memcpy(o + 12, I3, 72); memcpy(o + 21, T, 72); memcpy(o + 30, I3, 72);
    }
    auto mul = [](const double* A, const double* B, double* C) {   // C = A B (3 x 3 row-major)
        for (int i = 0; i < 3; i++) for (int j = 0; j < 3; j++) C[3 * i + j] = A[3 * i] * B[j] + A[3 * i + 1] * B[3 + j] + A[3 * i + 2] * B[6 + j];
    };
    auto mv = [](const double* A, const double* x, double* y) { for (int i = 0; i < 3; i++) y[i] = A[3 * i] * x[0] + A[3 * i + 1] * x[1] + A[3 * i + 2] * x[2]; };
    const double* T0 = pb->cam_T_s_f + 12 * (size_t)pb->cam0;
    const double* Tf = pb->frame_T_f_w;
    double Rcw[9], tcw[3], R0t[9], Rt[9];
    mul(T0, Tf, Rcw); mv(T0, Tf + 9, tcw);
    for (int a = 0; a < 3; a++) tcw[a] += T0[9 + a];                               // T_cam0_w = T_s_f(cam0) T_f_w(f)
    for (int i = 0; i < 3; i++) for (int j = 0; j < 3; j++) { R0t[3 * i + j] = T0[3 * j + i]; Rt[3 * i + j] = Tm[3 * j + i]; }
    for (int c = 0; c < nc; c++) {
        const double* Ts = pb->cam_T_s_f + 12 * (size_t)c;
        double Rc[9], tc[3], q[3], B[9];
        mul(Ts, R0t, Rc); mv(Rc, T0 + 9, q);
        for (int a = 0; a < 3; a++) tc[a] = Ts[9 + a] - q[a];                         // T_cam_cam0 = T_s_f(c) T_s_f(cam0)^-1
        mul(Rc, Rt, B);                                                               // Rc R^T
        double* o = &ctab[NOFOV_CTAB * (size_t)c];
        mul(B, Rcw, o);
        mv(B, tcw, o + 9);
        for (int a = 0; a < 3; a++) o[9 + a] += tc[a];
        mv(B, Tm + 9, o + 12);
    }
    NoFovDev P{};
    P.n_lmk = n; P.fixed = fixed; P.info = pb->info_scale; P.gate = pb->gate; P.huber_a = opts->huber_a;
    P.o.max_num_iterations = opts->max_num_iterations; P.o.jacobi_scaling = opts->jacobi_scaling;
    P.o.max_num_consecutive_invalid_steps = opts->max_num_consecutive_invalid_steps;
    P.o.function_tolerance = opts->function_tolerance; P.o.gradient_tolerance = opts->gradient_tolerance;
    P.o.parameter_tolerance = opts->parameter_tolerance; P.o.initial_radius = opts->initial_trust_region_radius;
    P.o.max_radius = opts->max_trust_region_radius; P.o.min_radius = opts->min_trust_region_radius;
    P.o.min_lm_diagonal = opts->min_lm_diagonal; P.o.max_lm_diagonal = opts->max_lm_diagonal; P.o.min_relative_decrease = opts->min_relative_decrease;
    // one allocation: header | ftab | ftsf | ctab | lmk_p | sbear | obear | out | scratch | scam | optr | ofr | ocam
    const size_t n_out = NOFOV_OUT * (size_t)n + NOFOV_SUM;
    const size_t n_d = ftab.size() + 12 * (size_t)nc + ctab.size() + 6 * (size_t)n + 3 * (size_t)no + n_out + NOFOV_LS * (size_t)n;
    const size_t n_i = (size_t)n + (size_t)n + 1 + 2 * (size_t)no;
    const size_t hdr = (sizeof(NoFovDev) + 15) & ~(size_t)15;
    DevBuf<char> buf;
    HIP_TRY(buf.alloc(hdr + 8 * n_d + 4 * n_i + 64));
    char* base = buf.p;
    double* dft = (double*)(base + hdr); double* dts = dft + ftab.size(); double* dct = dts + 12 * (size_t)nc;
    double* dlp = dct + ctab.size(); double* dsb = dlp + 3 * (size_t)n; double* dob = dsb + 3 * (size_t)n;
    double* dout = dob + 3 * (size_t)no; double* dscr = dout + n_out;
    int* dsc = (int*)(dscr + NOFOV_LS * (size_t)n); int* dptr = dsc + n; int* dofr = dptr + n + 1; int* docam = dofr + no;
    P.ftab = dft; P.ftsf = dts; P.ctab = dct; P.lmk_p = dlp; P.sbear = dsb; P.obear = dob; P.out = dout; P.scratch = dscr;
    P.scam = dsc; P.optr = dptr; P.ofr = dofr; P.ocam = docam;
    std::vector<int> zero_ptr(1, 0);
    HIP_TRY(hipMemcpyAsync(base, &P, sizeof(P), hipMemcpyHostToDevice, h->stream));
    HIP_TRY(hipMemcpyAsync(dft, ftab.data(), 8 * ftab.size(), hipMemcpyHostToDevice, h->stream));
    HIP_TRY(hipMemcpyAsync(dts, pb->cam_T_s_f, 96 * (size_t)nc, hipMemcpyHostToDevice, h->stream));
    HIP_TRY(hipMemcpyAsync(dct, ctab.data(), 8 * ctab.size(), hipMemcpyHostToDevice, h->stream));
    if (n) {
        HIP_TRY(hipMemcpyAsync(dlp, pb->lmk_p, 24 * (size_t)n, hipMemcpyHostToDevice, h->stream));
        HIP_TRY(hipMemcpyAsync(dsb, pb->scale_bearing, 24 * (size_t)n, hipMemcpyHostToDevice, h->stream));
        HIP_TRY(hipMemcpyAsync(dsc, pb->scale_cam, 4 * (size_t)n, hipMemcpyHostToDevice, h->stream));
        HIP_TRY(hipMemcpyAsync(dptr, pb->lmk_obs_ptr, 4 * ((size_t)n + 1), hipMemcpyHostToDevice, h->stream));
    } else HIP_TRY(hipMemcpyAsync(dptr, zero_ptr.data(), 4, hipMemcpyHostToDevice, h->stream));
    if (no) {
        HIP_TRY(hipMemcpyAsync(dob, pb->obs_bearing, 24 * (size_t)no, hipMemcpyHostToDevice, h->stream));
        HIP_TRY(hipMemcpyAsync(dofr, pb->obs_frame, 4 * (size_t)no, hipMemcpyHostToDevice, h->stream));
        HIP_TRY(hipMemcpyAsync(docam, pb->obs_cam, 4 * (size_t)no, hipMemcpyHostToDevice, h->stream));
    }
    hipLaunchKernelGGL(k_nofov, dim3(1), dim3(NOFOV_THREADS), 0, h->stream, (const NoFovDev*)base);
    HIP_TRY(hipGetLastError());
    std::vector<double> out(n_out);
    HIP_TRY(hipMemcpyAsync(out.data(), dout, 8 * n_out, hipMemcpyDeviceToHost, h->stream));
    HIP_TRY(hipStreamSynchronize(h->stream));
    const double* s = out.data() + NOFOV_OUT * (size_t)n;
    sadvio_solve_summary S{};
    S.initial_cost = s[0]; S.final_cost = s[1]; S.final_radius = s[2]; S.iterations = (int)s[3]; S.termination = (int)s[4];
    S.num_successful_steps = (int)s[5]; S.num_unsuccessful_steps = (int)s[6];
    const double lam = s[7];
    const bool usable = S.termination != SADVIO_TERM_FAILURE && lam >= 0.5 && lam <= 1.5;   // :870-871
    int n_in = 0;
    for (int l = 0; l < n; l++) {
        const double* o = out.data() + NOFOV_OUT * (size_t)l;
        if (lmk_delta3) memcpy(lmk_delta3 + 3 * (size_t)l, o, 24);
        if (gate_norm) gate_norm[l] = o[3];
        if (inlier) inlier[l] = o[4] != 0.0 ? 1 : 0;
        n_in += o[4] != 0.0 ? 1 : 0;
    }
    if (sum) *sum = S;
    if (res) {
        memset(res, 0, sizeof(*res));
        res->lambda = lam; res->usable = usable ? 1 : 0; res->scale_fixed = fixed; res->n_inliers = n_in;
    }
    if (!usable) h->err = S.termination == SADVIO_TERM_FAILURE ? "nofov_scale: no usable solution" : "nofov_scale: lambda outside [0.5, 1.5]";
    return usable ? SADVIO_OK : SADVIO_E_NOT_USABLE;
}

}  // extern "C"

#include "cov_driver.h"   // below marg_driver.h: the inversion of S is the unpivoted Cholesky + triangular inverse of sparsify's route

extern "C" {

// ---- marginal covariances of a solved window (no reference counterpart as one call: Sigma_k of Marginalization::sparsifyVIO,
//      marginalization.cpp:259-262, and covdT of the ESKF, ESKFEstimator.cpp:180, are what the pipeline consumes) ----
int sadvio_ba_covariance(sadvio_ba_handle* h, int32_t w, const sadvio_cov_request* rq, double* kf_cov, double* pair_cov, double* lmk_cov,
                         int32_t* n_lmk_singular) {
    if (!h) return SADVIO_E_INVALID_ARG;
    if (!h->env.long_cov)   // (SADVIO_CFG_LONG_TRACK_COVARIANCE: served, cov_long_kernels.h)
        if (int rc = refuse_long(h, w, "covariance")) return rc;
    return cov_run(h, w, rq, kf_cov, pair_cov, lmk_cov, n_lmk_singular);
}

int sadvio_ba_set_window(sadvio_ba_handle* h, const sadvio_flat_window* window) { return sadvio_ba_set_windows(h, 1, window); }

}  // extern "C"

#include "cov_batch_driver.h"   // below cov_driver.h: an item above the LDS cap goes through its steps

extern "C" {

// ---- the covariances of many windows of the solved batch in one call ----
int sadvio_ba_covariance_batch(sadvio_ba_handle* h, int32_t n_item, sadvio_cov_batch_item* items) {
    if (!h) return SADVIO_E_INVALID_ARG;
    // (SADVIO_CFG_LONG_TRACK_BATCH with SADVIO_CFG_LONG_TRACK_COVARIANCE: served — k_covb_long / k_covb_lmk_long on the group path, and
    // the single call's steps, which the covariance flag gates, for DENSE, BAND, square-root and retried items)
    for (int i = 0; items && i < n_item && !(h->env.long_batch && h->env.long_cov); i++)
        if (int rc = refuse_long(h, items[i].w, "covariance_batch")) return rc;
    return covb_run(h, n_item, items);
}

}  // extern "C"

#include "cov_cross_driver.h"   // below cov_driver.h: its steps up to cov_landmarks are the single call's

extern "C" {

// ---- key-frame x landmark cross covariances and the innovation gate of candidate observations ----
int sadvio_ba_covariance_cross(sadvio_ba_handle* h, int32_t w, const sadvio_cov_cross_request* rq, double* cross_cov, double* innov_cov, double* maha2,
                               int32_t* status) {
    if (!h) return SADVIO_E_INVALID_ARG;
    if (!h->env.long_cov)
        if (int rc = refuse_long(h, w, "covariance_cross")) return rc;
    return covx_run(h, w, rq, cross_cov, innov_cov, maha2, status);
}

}  // extern "C"

#include "rel_driver.h"

extern "C" {

// ---- the relative-pose information of many key-frame pairs of one window in one call (no reference counterpart as one call: the
//      reference's marginalizeRelative takes one pair, …Analytic.cpp:665-809) ----
int sadvio_ba_marginalize_relative_batch(sadvio_ba_handle* h, int32_t w, int32_t n_pair, const int32_t* kf_a, const int32_t* kf_b, int32_t eig_cut_mode,
                                         double* inf36, double* Ak144, double* T_a_b, int32_t* n_shared, int32_t* status) {
    if (!h) return SADVIO_E_INVALID_ARG;
    if (!h->env.long_batch)
        if (int rc = refuse_long(h, w, "marginalize_relative_batch")) return rc;
    return rel_run(h, w, n_pair, kf_a, kf_b, eig_cut_mode, inf36, Ak144, T_a_b, n_shared, status);
}

int sadvio_ba_landmark_chi2(sadvio_ba_handle* h, int32_t w, const double* pose_delta6, const double* lmk_delta3, const double* image_wh,
                            double pixel_sigma, double* avg_chi2, int32_t* inlier) {
    if (!h) return SADVIO_E_INVALID_ARG;
    if (!h->uploaded) { h->err = "landmark_chi2 before set_windows"; return SADVIO_E_STATE; }
    if (h->defer) { h->err = "landmark_chi2 between begin_update and commit_update"; return SADVIO_E_STATE; }
    if (w < 0 || w >= (int)h->plan.wins.size()) { h->err = "landmark_chi2: window out of range"; return SADVIO_E_INVALID_ARG; }
    HIP_TRY(hipSetDevice(h->device));
    const WinDev& d = h->plan.wins[w].d;
    if (d.n_lmk == 0) return SADVIO_OK;
    const SrcWin& S = h->src[w];
    // image bounds per stored camera (identical cameras are stored once; they must agree on the image size)
    std::vector<double> wh(2 * (size_t)d.n_cam, -1.0);
    for (int c = 0; c < S.v.n_cam; c++) {
        const int u = S.cam_map[c];
        const double bw = image_wh ? image_wh[2 * c] : 2.0 * S.cam_K[4 * (size_t)c + 2], bh = image_wh ? image_wh[2 * c + 1] : 2.0 * S.cam_K[4 * (size_t)c + 3];
        if (wh[2 * u] >= 0.0 && (wh[2 * u] != bw || wh[2 * u + 1] != bh)) { h->err = "landmark_chi2: cameras with identical (K, T_s_f, sigma) differ in image size"; return SADVIO_E_INVALID_ARG; }
        wh[2 * u] = bw; wh[2 * u + 1] = bh;
    }
    // deltas live in scratch (the solved state of the handle stays readable): [wh | out | xp | xl]
    const size_t n_wh = 2 * (size_t)(d.cam_base + d.n_cam), n_xp = 6 * (size_t)d.n_kf, n_xl = 3 * (size_t)d.n_lmk;
    HIP_TRY(h->d_probe.alloc(n_wh + 2 * (size_t)d.n_lmk + n_xp + n_xl));
    double* d_wh = h->d_probe.p; double* d_out = d_wh + n_wh; double* d_sxp = d_out + 2 * (size_t)d.n_lmk; double* d_sxl = d_sxp + n_xp;
    HIP_TRY(hipMemsetAsync(d_sxp, 0, sizeof(double) * (n_xp + n_xl), h->stream));
    if (pose_delta6) HIP_TRY(hipMemcpyAsync(d_sxp, pose_delta6, sizeof(double) * n_xp, hipMemcpyHostToDevice, h->stream));
    if (lmk_delta3) HIP_TRY(hipMemcpyAsync(d_sxl, lmk_delta3, sizeof(double) * n_xl, hipMemcpyHostToDevice, h->stream));
    HIP_TRY(hipMemcpyAsync(d_wh + 2 * (size_t)d.cam_base, wh.data(), sizeof(double) * wh.size(), hipMemcpyHostToDevice, h->stream));
    SolveOpts o{};
    DevPtrs P = make_ptrs(h, o, 1);
    P.xp = d_sxp - 6 * (ptrdiff_t)d.kf_base; P.xl = d_sxl - 3 * (ptrdiff_t)d.lmk_base;  // the kernel indexes globally
    const int blocks = (d.n_lmk + 63) / 64;
    const double isig = pixel_sigma > 0.0 ? 1.0 / pixel_sigma : (h->plan.factor_type == SADVIO_FACTOR_PIXEL ? 0.0 : 1.0);  // 0: cam_isig
    if (h->plan.factor_type == SADVIO_FACTOR_PIXEL) hipLaunchKernelGGL(k_lmk_chi2<0>, dim3(blocks), dim3(64), 0, h->stream, P, w, d_wh, isig, d_out);
    else hipLaunchKernelGGL(k_lmk_chi2<1>, dim3(blocks), dim3(64), 0, h->stream, P, w, d_wh, isig, d_out);
    HIP_TRY(hipGetLastError());
    std::vector<double> hb(2 * (size_t)d.n_lmk);
    HIP_TRY(hipMemcpyAsync(hb.data(), d_out, sizeof(double) * hb.size(), hipMemcpyDeviceToHost, h->stream));
    HIP_TRY(hipStreamSynchronize(h->stream));
    for (int l = 0; l < d.n_lmk; l++) {
        if (avg_chi2) avg_chi2[l] = hb[2 * (size_t)l];
        if (inlier) inlier[l] = (hb[2 * (size_t)l + 1] >= 2.0 && !(hb[2 * (size_t)l] > 2.0)) ? 1 : 0;
    }
    return SADVIO_OK;
}

static_assert(CAM_PINHOLE == SADVIO_CAM_PINHOLE && CAM_FISHEYE_EQUIDISTANT == SADVIO_CAM_FISHEYE_EQUIDISTANT && CAM_FISHEYE_EQUISOLID == SADVIO_CAM_FISHEYE_EQUISOLID &&
              CAM_FISHEYE_STEREOGRAPHIC == SADVIO_CAM_FISHEYE_STEREOGRAPHIC && CAM_OMNI == SADVIO_CAM_OMNI && CAM_DOUBLE_SPHERE == SADVIO_CAM_DOUBLE_SPHERE,
              "device_math.h restates the SADVIO_CAM_* kinds");

int sadvio_ba_landmark_chi2_models(sadvio_ba_handle* h, int32_t w, const double* pose_delta6, const double* lmk_delta3, const sadvio_camera_model* models,
                                   const double* obs_uv, double pixel_sigma, double* avg_chi2, int32_t* inlier, double* obs_chi2) {
    if (!h) return SADVIO_E_INVALID_ARG;
    if (!h->uploaded) { h->err = "landmark_chi2_models before set_windows"; return SADVIO_E_STATE; }
    if (h->defer) { h->err = "landmark_chi2_models between begin_update and commit_update"; return SADVIO_E_STATE; }
    if (w < 0 || w >= (int)h->plan.wins.size()) { h->err = "landmark_chi2_models: window out of range"; return SADVIO_E_INVALID_ARG; }
    if (!models) { h->err = "landmark_chi2_models: null model table"; return SADVIO_E_INVALID_ARG; }
    const WinDev& d = h->plan.wins[w].d;
    const SrcWin& S = h->src[w];
    // model and image bounds per stored camera (identical cameras are stored once; they must agree on both)
    std::vector<double> wh(2 * (size_t)d.n_cam, -1.0);
    std::vector<CamModelDev> md(std::max(d.n_cam, 1));
    for (int c = 0; c < S.v.n_cam; c++) {
        const sadvio_camera_model& m = models[c];
        if (m.kind < SADVIO_CAM_PINHOLE || m.kind > SADVIO_CAM_DOUBLE_SPHERE) { h->err = "landmark_chi2_models: unknown camera kind"; return SADVIO_E_INVALID_ARG; }
        const int u = S.cam_map[c];
        CamModelDev q{};
        q.rmax = m.rmax; q.xi = m.xi; q.alpha = m.alpha; q.kind = m.kind; q.distortion = m.distortion;
        for (int i = 0; i < 4; i++) q.D[i] = m.D[i];
        if (wh[2 * u] >= 0.0 && (wh[2 * u] != m.width || wh[2 * u + 1] != m.height || memcmp(&md[u], &q, sizeof(q)))) {
            h->err = "landmark_chi2_models: cameras with identical (K, T_s_f, sigma) differ in model or image size"; return SADVIO_E_INVALID_ARG;
        }
        wh[2 * u] = m.width; wh[2 * u + 1] = m.height; md[u] = q;
    }
    if (d.n_lmk == 0) return SADVIO_OK;
    HIP_TRY(hipSetDevice(h->device));
    // scratch: [wh | models | uv | xp | xl | obs | out] (the solved state of the handle stays readable); everything up to obs is
    // staged on the host and goes up in ONE copy, obs | out come back in one. The tables hold this window's cameras only.
    constexpr size_t MD = sizeof(CamModelDev) / sizeof(double);
    const size_t n_wh = 2 * (size_t)d.n_cam, n_md = MD * (size_t)d.n_cam, n_ob = (size_t)d.n_obs, n_uv = obs_uv ? 2 * n_ob : 0;
    const size_t n_xp = 6 * (size_t)d.n_kf, n_xl = 3 * (size_t)d.n_lmk, n_out = 2 * (size_t)d.n_lmk, n_up = n_wh + n_md + n_uv + n_xp + n_xl + n_ob;
    HIP_TRY(h->d_probe.alloc(n_up + n_out));
    double* d_wh = h->d_probe.p; double* d_md = d_wh + n_wh; double* d_uv = d_md + n_md; double* d_sxp = d_uv + n_uv; double* d_sxl = d_sxp + n_xp;
    double* d_ob = d_sxl + n_xl;
    std::vector<double> up(n_up, 0.0);   // deltas NULL = zeros; obs = 0 where no landmark lists the observation
    memcpy(up.data(), wh.data(), sizeof(double) * n_wh);
    memcpy(up.data() + n_wh, md.data(), sizeof(double) * n_md);
    if (obs_uv)                          // the measured pixels in the stored observation order (obs_perm: stored position -> caller's index)
        for (int a = 0; a < d.n_obs; a++) {
            const int src = h->plan.obs_perm[d.obs_base + a];
            if (src >= 0) { up[n_wh + n_md + 2 * (size_t)a] = obs_uv[2 * (size_t)src]; up[n_wh + n_md + 2 * (size_t)a + 1] = obs_uv[2 * (size_t)src + 1]; }
        }
    if (pose_delta6) memcpy(up.data() + n_wh + n_md + n_uv, pose_delta6, sizeof(double) * n_xp);
    if (lmk_delta3) memcpy(up.data() + n_wh + n_md + n_uv + n_xp, lmk_delta3, sizeof(double) * n_xl);
    HIP_TRY(hipMemcpyAsync(d_wh, up.data(), sizeof(double) * n_up, hipMemcpyHostToDevice, h->stream));
    SolveOpts o{};
    DevPtrs P = make_ptrs(h, o, 1);
    P.xp = d_sxp - 6 * (ptrdiff_t)d.kf_base; P.xl = d_sxl - 3 * (ptrdiff_t)d.lmk_base;  // the kernel indexes globally
    const double* k_wh = d_wh - 2 * (ptrdiff_t)d.cam_base;                               // ... the camera tables too
    const CamModelDev* k_md = (const CamModelDev*)d_md - (ptrdiff_t)d.cam_base;
    const int blocks = (d.n_lmk + 63) / 64;
    const double isig = pixel_sigma > 0.0 ? 1.0 / pixel_sigma : (h->plan.factor_type == SADVIO_FACTOR_PIXEL ? 0.0 : 1.0);  // 0: cam_isig
    const double* k_uv = obs_uv ? d_uv : nullptr;
    if (h->plan.factor_type == SADVIO_FACTOR_PIXEL) hipLaunchKernelGGL(k_lmk_chi2_models<0>, dim3(blocks), dim3(64), 0, h->stream, P, w, k_wh, k_md, k_uv, isig, d_ob + n_ob, d_ob);
    else hipLaunchKernelGGL(k_lmk_chi2_models<1>, dim3(blocks), dim3(64), 0, h->stream, P, w, k_wh, k_md, k_uv, isig, d_ob + n_ob, d_ob);
    HIP_TRY(hipGetLastError());
    std::vector<double> hb(n_ob + n_out);   // obs | out
    HIP_TRY(hipMemcpyAsync(hb.data(), d_ob, sizeof(double) * hb.size(), hipMemcpyDeviceToHost, h->stream));
    HIP_TRY(hipStreamSynchronize(h->stream));
    const double* h_out = hb.data() + n_ob;
    for (int l = 0; l < d.n_lmk; l++) {
        if (avg_chi2) avg_chi2[l] = h_out[2 * (size_t)l];
        if (inlier) inlier[l] = (h_out[2 * (size_t)l + 1] >= 2.0 && !(h_out[2 * (size_t)l] > 2.0)) ? 1 : 0;
    }
    if (obs_chi2)
        for (int a = 0; a < d.n_obs; a++) {
            const int src = h->plan.obs_perm[d.obs_base + a];
            if (src >= 0) obs_chi2[src] = hb[(size_t)a];
        }
    return SADVIO_OK;
}

int sadvio_ba_get_kernel_times(sadvio_ba_handle* h, int32_t cap, const char** names, double* avg_us, int64_t* launches) {
    if (!h) return SADVIO_E_INVALID_ARG;
    int n = 0;
    for (auto& k : h->kclasses) {
        if (n >= cap) break;
        if (names) names[n] = k.name;
        if (avg_us) avg_us[n] = k.launches ? 1e3 * k.total_ms / (double)k.launches : 0.0;
        if (launches) launches[n] = k.launches;
        n++;
    }
    return n;
}

// (a NULL handle: why this thread's last sadvio_ba_create refused its configuration, if it did)
const char* sadvio_ba_last_error(sadvio_ba_handle* h) { return h ? h->err.c_str() : (create_err.empty() ? "null handle" : create_err.c_str()); }
const char* sadvio_ba_version(void) { return "sadvio-ba-mi355x 0.5 (gfx950)"; }

}  // extern "C"
