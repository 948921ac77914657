// factors_driver.h — what the setters keep of the caller's data: the deep copies of set_windows and the bodies of set_lines,
// set_pose_priors, set_imu_factors, set_dense_prior and set_sparse_priors. Each validates against the window's sizes, records its
// factors in the handle's per-window lists and, outside begin_update .. commit_update, rebuilds what it changes (layout_driver.h).
// The entry points (ba_capi.hip) have checked the handle's state, the window index and the counts.
// Part of the library's single translation unit (ba_capi.hip); not a public header.
#pragma once
#include "ba_handle.h"
#include "imu_host.h"
#include "layout_driver.h"

namespace {

// set_windows: deep copies (later set_* calls rebuild the layout without the caller's buffers), empty factor lists, then the layout
int keep_windows(sadvio_ba_handle* h, int32_t n_windows, const sadvio_flat_window* wins) {
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

int set_lines(sadvio_ba_handle* h, int32_t w, const sadvio_line_set* L) {
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

int set_pose_priors(sadvio_ba_handle* h, int32_t w, int32_t n, const sadvio_pose_prior* pr) {
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

int set_imu_factors(sadvio_ba_handle* h, int32_t w, int32_t n, const sadvio_imu_factor* fs) {
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
        if (!make_imu_dev(f, d.kf_base, o)) { h->err = "set_imu_factors: covariance is not positive definite"; return SADVIO_E_INVALID_ARG; }
        v.push_back(o);
    }
    if (h->defer) { h->pending = true; return SADVIO_OK; }
    h->up.reset();
    return upload_priors(h);
}

int set_dense_prior(sadvio_ba_handle* h, int32_t w, int32_t n_full, int32_t n, const double* J, const double* r0, int32_t kf_keep, int32_t kf_col,
                    int32_t n_keep, const int32_t* lmk_index, const int32_t* lmk_col) {
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

int set_sparse_priors(sadvio_ba_handle* h, int32_t w, int32_t n, const sadvio_sparse_prior* f) {
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
    if (h->lt.min > 0 && h->world == 1 && !h->coll_fn) {
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

}  // namespace
