// ba_capi.hip — the C ABI (include/sadvio_ba.h) of the MI355X BA backend: entry points only.
//
// Replaces, behind the reference's optimizer boundary, the body of AOptimizer::localMapBA /
// localMapVIOptimization from `ceres::Solve` on (AOptimizer.cpp:326,388): the windows are uploaded
// once (set_windows), the whole LM solve is enqueued on the handle's stream without host round
// trips, and deltas are read back for the adapter to apply (AOptimizer.cpp:329-340).
// There is no CPU fallback: without a gfx950 device every compute call fails.
//
// Every entry point checks its own arguments and the handle's state (entry_state, ba_handle.h), then calls one function of a driver
// header. The order of the checks inside an entry point decides which refusal a caller sees: it is part of the call's behaviour.
#include "ba_handle.h"
#include "comm_driver.h"
#include "cov_batch_driver.h"
#include "cov_cross_driver.h"
#include "cov_driver.h"
#include "factors_driver.h"
#include "gate_driver.h"
#include "layout_driver.h"
#include "marg_driver.h"
#include "nofov_driver.h"
#include "rel_driver.h"
#include "solve_driver.h"
#include "viinit_driver.h"

namespace {
// why sadvio_ba_create refused its configuration: there is no handle to hold the text, sadvio_ba_last_error(NULL) returns it
thread_local std::string create_err;
// is w a window of the current layout
bool has_window(const sadvio_ba_handle* h, int w) { return w >= 0 && w < (int)h->plan.wins.size(); }
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
    EnvCfg env;
    env.read();
    LongCfg lt;
    if (!lt.from_create(cfg ? cfg->reserved : 0, env.long_min_env, create_err)) return SADVIO_E_INVALID_ARG;
    int n = 0;
    if (hipGetDeviceCount(&n) != hipSuccess || n == 0) return SADVIO_E_NO_DEVICE;
    int dev = cfg ? cfg->device : 0;
    if (dev < 0 || dev >= n) return SADVIO_E_INVALID_ARG;
    hipDeviceProp_t prop;
    if (hipGetDeviceProperties(&prop, dev) != hipSuccess) return SADVIO_E_HIP;
    if (!strstr(prop.gcnArchName, "gfx950")) return SADVIO_E_NO_DEVICE;  // kernels are built for gfx950 only
    if (hipSetDevice(dev) != hipSuccess) return SADVIO_E_HIP;
    auto* h = new sadvio_ba_handle();
    h->env = env; h->lt = lt;
    h->up.trace = (h->env.debug & 8192) != 0;
    if (cfg) h->cfg = *cfg;
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
    return keep_windows(h, n_windows, wins);
}

int sadvio_ba_set_window(sadvio_ba_handle* h, const sadvio_flat_window* window) { return sadvio_ba_set_windows(h, 1, window); }

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
    if (int rc = entry_state(h, "set_lines", NEED_UPLOADED)) return rc;
    if (!has_window(h, w)) { h->err = "set_lines: window out of range"; return SADVIO_E_INVALID_ARG; }
    return set_lines(h, w, L);
}

int sadvio_ba_get_line_deltas(sadvio_ba_handle* h, int32_t w, double* line_delta6) {
    if (!h) return SADVIO_E_INVALID_ARG;
    if (int rc = entry_state(h, "get_line_deltas", NEED_SOLVED)) return rc;
    if (!has_window(h, w) || !line_delta6) { h->err = "get_line_deltas: bad argument"; return SADVIO_E_INVALID_ARG; }
    return read_line_deltas(h, w, line_delta6);
}

int sadvio_ba_set_pose_priors(sadvio_ba_handle* h, int32_t w, int32_t n, const sadvio_pose_prior* pr) {
    if (!h) return SADVIO_E_INVALID_ARG;
    if (int rc = entry_state(h, "set_pose_priors", NEED_UPLOADED)) return rc;
    if (!has_window(h, w) || n < 0 || (n > 0 && !pr)) { h->err = "set_pose_priors: bad argument"; return SADVIO_E_INVALID_ARG; }
    return set_pose_priors(h, w, n, pr);
}

int sadvio_ba_set_imu_factors(sadvio_ba_handle* h, int32_t w, int32_t n, const sadvio_imu_factor* fs) {
    if (!h) return SADVIO_E_INVALID_ARG;
    if (int rc = entry_state(h, "set_imu_factors", NEED_UPLOADED)) return rc;
    if (!has_window(h, w) || n < 0 || (n > 0 && !fs)) { h->err = "set_imu_factors: bad argument"; return SADVIO_E_INVALID_ARG; }
    return set_imu_factors(h, w, n, fs);
}

int sadvio_ba_set_dense_prior(sadvio_ba_handle* h, int32_t w, int32_t n_full, int32_t n, const double* J, const double* r0,
                              int32_t kf_keep, int32_t kf_col, int32_t n_keep, const int32_t* lmk_index, const int32_t* lmk_col) {
    if (!h) return SADVIO_E_INVALID_ARG;
    if (int rc = entry_state(h, "set_dense_prior", NEED_UPLOADED)) return rc;
    if (!has_window(h, w) || (n_full < 0 && n_full != SADVIO_PRIOR_RESIDENT) || (n < 0 && n_full != SADVIO_PRIOR_RESIDENT) || n_keep < 0) { h->err = "set_dense_prior: bad argument"; return SADVIO_E_INVALID_ARG; }
    return set_dense_prior(h, w, n_full, n, J, r0, kf_keep, kf_col, n_keep, lmk_index, lmk_col);
}

int sadvio_ba_set_sparse_priors(sadvio_ba_handle* h, int32_t w, int32_t n, const sadvio_sparse_prior* f) {
    if (!h) return SADVIO_E_INVALID_ARG;
    if (int rc = entry_state(h, "set_sparse_priors", NEED_UPLOADED)) return rc;
    if (!has_window(h, w) || n < 0 || (n > 0 && !f)) { h->err = "set_sparse_priors: bad argument"; return SADVIO_E_INVALID_ARG; }
    return set_sparse_priors(h, w, n, f);
}

int sadvio_ba_marginalize(sadvio_ba_handle* h, int32_t w, const sadvio_marg_request* rq, sadvio_marg_result* res, int32_t* lmk_col_out,
                          double* J_out, double* r0_out) {
    if (!h) return SADVIO_E_INVALID_ARG;
    if (int rc = entry_state(h, "marginalize", NEED_UPLOADED | NOT_DEFERRED)) return rc;
    if (!rq || !has_window(h, w)) { h->err = "marginalize: bad argument"; return SADVIO_E_INVALID_ARG; }
    if (h->world > 1) { h->err = "marginalize: the window is sharded over several GPUs (each rank holds a landmark partition only)"; return SADVIO_E_INVALID_ARG; }
    // (SADVIO_CFG_LONG_TRACK_PRIORS: served. marg_layout lists one item per observation from lmk_ob / lmk_oe / obs_perm, which hold a long
    // track's observations like any others, and k_marg_obs takes an item by its device index: nothing there walks a lane group)
    if (!h->lt.priors)
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

int sadvio_ba_one_round(sadvio_ba_handle* h, int32_t* taken) {
    if (!h || !taken) return SADVIO_E_INVALID_ARG;
    *taken = h->last_one_round ? 1 : 0;
    return SADVIO_OK;
}

int sadvio_ba_get_prior(sadvio_ba_handle* h, sadvio_prior_info* info, double* J, double* r0) {
    if (!h) return SADVIO_E_INVALID_ARG;
    return read_prior(h, info, J, r0);
}

int sadvio_ba_set_prior(sadvio_ba_handle* h, int32_t n_full, int32_t n, int32_t form, const double* J, const double* r0) {
    if (!h) return SADVIO_E_INVALID_ARG;
    return write_prior(h, n_full, n, form, J, r0);
}

int sadvio_ba_marginalize_relative(sadvio_ba_handle* h, int32_t w, int32_t kf_a, int32_t kf_b, int32_t eig_cut_mode, double* inf36, double* Ak144) {
    if (!h || !inf36) return SADVIO_E_INVALID_ARG;
    if (int rc = entry_state(h, "marginalize_relative", NEED_UPLOADED | NOT_DEFERRED)) return rc;
    if (!has_window(h, w)) { h->err = "marginalize_relative: window out of range"; return SADVIO_E_INVALID_ARG; }
    if (eig_cut_mode != SADVIO_EIG_CUT_REFERENCE && eig_cut_mode != SADVIO_EIG_CUT_NOISE_FLOOR) { h->err = "marginalize_relative: bad eig_cut_mode"; return SADVIO_E_INVALID_ARG; }
    if (h->world > 1) { h->err = "marginalize_relative: the window is sharded over several GPUs (each rank holds a landmark partition only)"; return SADVIO_E_INVALID_ARG; }
    const WinDev& d = h->plan.wins[w].d;
    if (kf_a < 0 || kf_a >= d.n_kf || kf_b < 0 || kf_b >= d.n_kf || kf_a == kf_b) { h->err = "marginalize_relative: bad key-frame index"; return SADVIO_E_INVALID_ARG; }
    if (!h->lt.batch)   // (SADVIO_CFG_LONG_TRACK_BATCH: served; a long track's observations are found by bisection, rel_runs.h)
        if (int rc = refuse_long(h, w, "marginalize_relative")) return rc;
    if (d.has_imu) { h->err = "marginalize_relative: frames with IMU states are not supported (the reference's own column layout for them is inconsistent, BundleAdjustmentCERESAnalytic.cpp:705-737)"; return SADVIO_E_INVALID_ARG; }
    return marginalize_relative(h, w, kf_a, kf_b, eig_cut_mode, inf36, Ak144);
}

// ---- the relative-pose information of many key-frame pairs of one window in one call (no reference counterpart as one call: the
//      reference's marginalizeRelative takes one pair, …Analytic.cpp:665-809) ----
int sadvio_ba_marginalize_relative_batch(sadvio_ba_handle* h, int32_t w, int32_t n_pair, const int32_t* kf_a, const int32_t* kf_b, int32_t eig_cut_mode,
                                         double* inf36, double* Ak144, double* T_a_b, int32_t* n_shared, int32_t* status) {
    if (!h) return SADVIO_E_INVALID_ARG;
    if (!h->lt.batch)
        if (int rc = refuse_long(h, w, "marginalize_relative_batch")) return rc;
    return rel_run(h, w, n_pair, kf_a, kf_b, eig_cut_mode, inf36, Ak144, T_a_b, n_shared, status);
}

int sadvio_ba_sparsify(sadvio_ba_handle* h, int32_t w, int32_t vio, int32_t nf, int32_t n, const double* J, int32_t kf_keep,
                       int32_t kf_col, int32_t n_keep, const int32_t* lmk_index, const int32_t* lmk_col, int32_t* n_out,
                       sadvio_sparse_prior* out) {
    if (!h) return SADVIO_E_INVALID_ARG;
    if (n_out) *n_out = 0;
    if (int rc = entry_state(h, "sparsify", NEED_UPLOADED | NOT_DEFERRED)) return rc;
    if (!has_window(h, w) || !n_out || !out || n_keep < 0 || (n_keep > 0 && (!lmk_index || !lmk_col))) { h->err = "sparsify: bad argument"; return SADVIO_E_INVALID_ARG; }
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

int sadvio_ba_rccl_unique_id(void* id128) {
    if (!id128) return SADVIO_E_INVALID_ARG;
    return rccl_unique_id(id128);
}

int sadvio_ba_comm_init_rccl(sadvio_ba_handle* h, int32_t rank, int32_t world, const void* id128) {
    if (!h) return SADVIO_E_INVALID_ARG;
    if (!id128 || world < 1 || rank < 0 || rank >= world) { h->err = "comm_init_rccl: bad argument"; return SADVIO_E_INVALID_ARG; }
    if (h->uploaded) { h->err = "comm_init_rccl must precede set_windows"; return SADVIO_E_STATE; }
    return comm_init_rccl(h, rank, world, id128);
}

int sadvio_ba_comm_info(sadvio_ba_handle* h, int32_t* nranks, int32_t* rank, int32_t* device, int32_t* is_rccl) {
    if (!h) return SADVIO_E_INVALID_ARG;
    return comm_info(h, nranks, rank, device, is_rccl);
}

int sadvio_ba_solve(sadvio_ba_handle* h, const sadvio_solve_options* opts, sadvio_solve_summary* summaries) {
    if (!h) return SADVIO_E_INVALID_ARG;
    if (int rc = entry_state(h, "solve", NEED_UPLOADED | NOT_DEFERRED)) return rc;
    // 1. options
    SolveOpts o;
    if (int rc = convert_options(h, opts, o)) return rc;
    HIP_TRY(hipSetDevice(h->device));
    // 2. plan: everything the launch sequence reads
    SolvePlan plan;
    std::vector<BigPlan> big;
    if (int rc = plan_solve(h, o, plan, big)) return rc;
    // 3. launch, as one graph where the handle asks for it
    if (int rc = launch_solve(h, plan, big)) return rc;
    // 4. wait, collect the timers
    HIP_TRY(hipStreamSynchronize(h->stream));
    if (h->cfg.profile_kernels) collect_timers(h);
    // 5. diagnostics
    if (h->env.debug & 4096) print_debug_stamps(h, plan.P.n_tiles);
    // 6. summaries
    return solve_summaries(h, o, plan, summaries);
}

int sadvio_ba_get_deltas(sadvio_ba_handle* h, int32_t w, double* pose, double* lmk, double* dv, double* dba, double* dbg) {
    if (!h) return SADVIO_E_INVALID_ARG;
    if (int rc = entry_state(h, "get_deltas", NEED_SOLVED)) return rc;
    if (!has_window(h, w)) { h->err = "get_deltas: window out of range"; return SADVIO_E_INVALID_ARG; }
    return read_deltas(h, w, pose, lmk, dv, dba, dbg);
}

int sadvio_ba_get_trace(sadvio_ba_handle* h, int32_t w, int32_t cap_rows, double* rows8, int32_t* n_rows) {
    if (!h) return SADVIO_E_INVALID_ARG;
    if (int rc = entry_state(h, "get_trace", NEED_SOLVED)) return rc;
    if (!has_window(h, w) || cap_rows < 0 || (cap_rows > 0 && !rows8)) { h->err = "get_trace: bad argument"; return SADVIO_E_INVALID_ARG; }
    return read_trace(h, w, cap_rows, rows8, n_rows);
}

int sadvio_ba_get_ids(sadvio_ba_handle* h, int32_t w, int64_t* kf_id, int64_t* lmk_id) {
    if (!h) return SADVIO_E_INVALID_ARG;
    if (!has_window(h, w)) { h->err = "get_ids: window out of range"; return SADVIO_E_INVALID_ARG; }
    if (kf_id) memcpy(kf_id, h->plan.wins[w].kf_id.data(), sizeof(int64_t) * h->plan.wins[w].kf_id.size());
    if (lmk_id) memcpy(lmk_id, h->plan.wins[w].lmk_id.data(), sizeof(int64_t) * h->plan.wins[w].lmk_id.size());
    return SADVIO_OK;
}

int sadvio_ba_linearize(sadvio_ba_handle* h, int32_t w, const double* pose_delta6, const double* lmk_delta3, double* r2,
                        double* Jp12, double* Jl6) {
    if (!h) return SADVIO_E_INVALID_ARG;
    if (int rc = entry_state(h, "linearize", NEED_UPLOADED | NOT_DEFERRED)) return rc;
    if (!has_window(h, w)) { h->err = "linearize: window out of range"; return SADVIO_E_INVALID_ARG; }
    return linearize(h, w, pose_delta6, lmk_delta3, r2, Jp12, Jl6);
}

int sadvio_ba_landmark_chi2(sadvio_ba_handle* h, int32_t w, const double* pose_delta6, const double* lmk_delta3, const double* image_wh,
                            double pixel_sigma, double* avg_chi2, int32_t* inlier) {
    if (!h) return SADVIO_E_INVALID_ARG;
    if (int rc = entry_state(h, "landmark_chi2", NEED_UPLOADED | NOT_DEFERRED)) return rc;
    if (!has_window(h, w)) { h->err = "landmark_chi2: window out of range"; return SADVIO_E_INVALID_ARG; }
    return landmark_chi2(h, w, pose_delta6, lmk_delta3, image_wh, pixel_sigma, avg_chi2, inlier);
}

int sadvio_ba_landmark_chi2_models(sadvio_ba_handle* h, int32_t w, const double* pose_delta6, const double* lmk_delta3, const sadvio_camera_model* models,
                                   const double* obs_uv, double pixel_sigma, double* avg_chi2, int32_t* inlier, double* obs_chi2) {
    if (!h) return SADVIO_E_INVALID_ARG;
    if (int rc = entry_state(h, "landmark_chi2_models", NEED_UPLOADED | NOT_DEFERRED)) return rc;
    if (!has_window(h, w)) { h->err = "landmark_chi2_models: window out of range"; return SADVIO_E_INVALID_ARG; }
    if (!models) { h->err = "landmark_chi2_models: null model table"; return SADVIO_E_INVALID_ARG; }
    return landmark_chi2_models(h, w, pose_delta6, lmk_delta3, models, obs_uv, pixel_sigma, avg_chi2, inlier, obs_chi2);
}

int sadvio_ba_vi_init(sadvio_ba_handle* h, const sadvio_viinit_problem* pb, const sadvio_solve_options* opts, sadvio_solve_summary* sum,
                      sadvio_viinit_result* res, double* dv3) {
    if (!h) return SADVIO_E_INVALID_ARG;
    if (!pb || !opts || pb->n_frames < 0 || pb->n_factors < 0 || (pb->n_frames > 0 && (!pb->T_f_w || !pb->vel)) || (pb->n_factors > 0 && !pb->factors)) {
        h->err = "vi_init: bad argument"; return SADVIO_E_INVALID_ARG;
    }
    if (pb->n_frames > VIINIT_MAX_FRAMES) { h->err = "vi_init: more than 48 frames"; return SADVIO_E_INVALID_ARG; }
    if (pb->optim_bias && !(pb->sigma_dba > 0.0 && pb->sigma_dbg > 0.0)) { h->err = "vi_init: bias prior sigmas must be positive"; return SADVIO_E_INVALID_ARG; }
    return vi_init(h, pb, opts, sum, res, dv3);
}

// (landmarkOptimizationNoFov: nofov_plan.h holds the argument checks, so that they run without a device)
int sadvio_ba_nofov_scale(sadvio_ba_handle* h, const sadvio_nofov_problem* pb, const sadvio_solve_options* opts, sadvio_solve_summary* sum,
                          sadvio_nofov_result* res, double* lmk_delta3, double* gate_norm, int32_t* inlier) {
    if (!h) return SADVIO_E_INVALID_ARG;
    return nofov_scale(h, pb, opts, sum, res, lmk_delta3, gate_norm, inlier);
}

// ---- marginal covariances of a solved window (no reference counterpart as one call: Sigma_k of Marginalization::sparsifyVIO,
//      marginalization.cpp:259-262, and covdT of the ESKF, ESKFEstimator.cpp:180, are what the pipeline consumes) ----
int sadvio_ba_covariance(sadvio_ba_handle* h, int32_t w, const sadvio_cov_request* rq, double* kf_cov, double* pair_cov, double* lmk_cov,
                         int32_t* n_lmk_singular) {
    if (!h) return SADVIO_E_INVALID_ARG;
    if (!h->lt.cov)   // (SADVIO_CFG_LONG_TRACK_COVARIANCE: served, cov_long_kernels.h)
        if (int rc = refuse_long(h, w, "covariance")) return rc;
    return cov_run(h, w, rq, kf_cov, pair_cov, lmk_cov, n_lmk_singular);
}

// ---- the covariances of many windows of the solved batch in one call ----
int sadvio_ba_covariance_batch(sadvio_ba_handle* h, int32_t n_item, sadvio_cov_batch_item* items) {
    if (!h) return SADVIO_E_INVALID_ARG;
    // (SADVIO_CFG_LONG_TRACK_BATCH with SADVIO_CFG_LONG_TRACK_COVARIANCE: served — k_covb_long / k_covb_lmk_long on the group path, and
    // the single call's steps, which the covariance flag gates, for DENSE, BAND, square-root and retried items)
    for (int i = 0; items && i < n_item && !(h->lt.batch && h->lt.cov); i++)
        if (int rc = refuse_long(h, items[i].w, "covariance_batch")) return rc;
    return covb_run(h, n_item, items);
}

// ---- key-frame x landmark cross covariances and the innovation gate of candidate observations ----
int sadvio_ba_covariance_cross(sadvio_ba_handle* h, int32_t w, const sadvio_cov_cross_request* rq, double* cross_cov, double* innov_cov, double* maha2,
                               int32_t* status) {
    if (!h) return SADVIO_E_INVALID_ARG;
    if (!h->lt.cov)
        if (int rc = refuse_long(h, w, "covariance_cross")) return rc;
    return covx_run(h, w, rq, cross_cov, innov_cov, maha2, status);
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
