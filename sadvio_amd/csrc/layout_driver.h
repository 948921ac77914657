// layout_driver.h — the device half of a layout: layout_plan.h decides every table on the host, the functions here allocate, zero what
// the kernels expect zeroed, queue the plan's arrays in the handle's upload batch and launch the few kernels that finish the upload
// (dense-prior J^T and J^T J, first-round packets). Planning is finished before the first h->up.add, so a refused layout queues nothing.
// Part of the library's single translation unit (ba_capi.hip).
#pragma once
#include "ba_handle.h"

namespace {

// J^T of a dense prior, once per upload (J is constant during the solve); H = J^T J is a k_mgemm launch (FP64 matrix cores:
// the one-thread-per-entry loop this replaces took 0.92 ms at n = 915, more than the layout build itself).
__global__ void k_dense_prior_prepare(const double* J, double* Jt, int nf, int n) {
    const long long idx = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (idx < (long long)nf * n) {
        const int i = (int)(idx / n), a = (int)(idx - (long long)i * n);
        Jt[(size_t)a * nf + i] = J[idx];
    }
}

// H = the symmetric matrix whose lower triangle is A's (the marginalisation's Ak, read like Eigen reads it)
__global__ void k_sym_from_lower(const double* __restrict__ A, int n, double* __restrict__ H) {
    const long long idx = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (idx >= (long long)n * n) return;
    const int i = (int)(idx / n), j = (int)(idx - (long long)i * n);
    H[idx] = i >= j ? A[idx] : A[(size_t)j * n + i];
}

LayoutIn layout_inputs(sadvio_ba_handle* h) {
    LayoutIn in;
    in.src = &h->src; in.sparse_per_win = &h->sparse_per_win; in.dprior_per_win = &h->dprior_per_win; in.lines_per_win = &h->lines_per_win;
    in.prior_valid = h->prior.valid; in.prior_serial = h->prior.serial; in.prior_n_full = h->prior.n_full; in.prior_n = h->prior.n;
    in.world = h->world; in.has_coll = h->coll_fn != nullptr;
    in.tile_rounds = h->env.tile_rounds; in.lm = h->env.lm; in.lm_subs = h->env.lm_subs;
    in.contig_tiles = h->env.contig_tiles; in.no_lpt = h->env.no_lpt; in.no_pre = h->env.no_pre;
    in.long_min = h->lt.min; in.long_priors = h->lt.priors;
    return in;
}

// queue a host table for the device buffer that holds it
template <typename T>
void queue_table(sadvio_ba_handle* h, DevBuf<T>& dst, const std::vector<T>& src) { h->up.add(dst.p, src.data(), src.size() * sizeof(T)); }

// The planned reduced systems on the device: the buffer of the per-step all-reduce, the factor tables, the dense priors' data.
int layout_reduced_device(sadvio_ba_handle* h) {
    LayoutPlan& P = h->plan;
    const long long s_b = P.s_tot, nrb = P.n_rank_b;
    const int red_b = P.np_tot;
    // one allocation [S | gred | gfull | hdiag | rank_b]: a window sharded over several GPUs all-reduces it whole
    HIP_TRY(h->d_S.alloc((size_t)std::max<long long>(P.red_total, 1)));
    h->d_gred.set_view(h->d_S.p + s_b, (size_t)red_b); h->d_gfull.set_view(h->d_gred.p + red_b, (size_t)red_b);
    h->d_hdiag.set_view(h->d_gfull.p + red_b, (size_t)red_b); h->d_rank_b.set_view(h->d_hdiag.p + red_b, (size_t)nrb);
    HIP_TRY(h->d_rank_s.alloc((size_t)nrb));
    HIP_TRY(h->d_delta.alloc((size_t)std::max(red_b, 1))); HIP_TRY(h->d_s_pose.alloc((size_t)std::max(red_b, 1)));
    HIP_TRY(hipMemsetAsync(h->d_S.p, 0, sizeof(double) * (size_t)std::max<long long>(P.red_total, 1), h->stream));
    HIP_TRY(hipMemsetAsync(h->d_rank_s.p, 0, sizeof(double) * (size_t)nrb, h->stream));
    HIP_TRY(h->d_sparse.alloc(std::max<size_t>(P.sparse.size(), 1))); HIP_TRY(h->d_sp_scratch.alloc(2 * std::max<size_t>(P.sparse.size(), 1) * SPARSE_J));
    HIP_TRY(h->d_sp_list.alloc(std::max<size_t>(P.sp_list.size(), 1)));
    h->n_sparse_tot = P.sparse.size(); h->n_sp_list = (int)P.sp_list.size();
    h->n_line_tot = (int)P.lines.size(); h->n_lobs_tot = (int)P.lobs.size();
    HIP_TRY(h->d_lines.alloc(std::max<size_t>(P.lines.size(), 1))); HIP_TRY(h->d_lobs.alloc(std::max<size_t>(P.lobs.size(), 1)));
    HIP_TRY(h->d_xline.alloc(std::max<size_t>(12 * P.lines.size(), 1))); HIP_TRY(h->d_line_scratch.alloc(std::max<size_t>(P.lobs.size(), 1) * LINE_ROW));
    HIP_TRY(h->d_tiles.alloc(P.tiles.size())); HIP_TRY(h->d_lmk_red.alloc(P.lmk_red.size())); HIP_TRY(h->d_lmk_const.alloc(P.lmk_const_red.size()));
    HIP_TRY(h->d_kept_obs.alloc(P.kept.size())); HIP_TRY(h->d_dp_ints.alloc(P.dp_ints.size())); HIP_TRY(h->d_dp_data.alloc((size_t)std::max<long long>(P.dp_total, 1)));
    queue_table(h, h->d_sparse, P.sparse); queue_table(h, h->d_sp_list, P.sp_list); queue_table(h, h->d_lines, P.lines); queue_table(h, h->d_lobs, P.lobs);
    queue_table(h, h->d_tiles, P.tiles); queue_table(h, h->d_lmk_red, P.lmk_red); queue_table(h, h->d_lmk_const, P.lmk_const_red);
    queue_table(h, h->d_kept_obs, P.kept); queue_table(h, h->d_dp_ints, P.dp_ints);
    // the dense priors' data never exists as one host array: scratch parts are zeroed on the device, J and r0 come from the
    // caller's copy (staged upload) or from the handle's prior (device to device, no PCIe traffic)
    if (!P.preps.empty()) HIP_TRY(hipMemsetAsync(h->d_dp_data.p, 0, sizeof(double) * (size_t)P.dp_total, h->stream));
    for (const DensePrep& pr : P.preps) {
        const DensePriorHost& D = h->dprior_per_win[pr.w];
        double* J = h->d_dp_data.p + pr.off;
        double* r0 = J + 2 * (size_t)pr.nf * pr.n + (size_t)pr.n * pr.n;
        if (D.resident) {   // (the plan checked that the handle's prior is still the one the window attached)
            HIP_TRY(hipMemcpyAsync(J, h->prior.J.p, sizeof(double) * (size_t)pr.nf * pr.n, hipMemcpyDeviceToDevice, h->stream));
            HIP_TRY(hipMemcpyAsync(r0, h->prior.r0.p, sizeof(double) * (size_t)pr.nf, hipMemcpyDeviceToDevice, h->stream));
        } else {
            h->up.add(J, D.J.data(), sizeof(double) * (size_t)pr.nf * pr.n);
            h->up.add(r0, D.r0.data(), sizeof(double) * (size_t)pr.nf);
        }
    }
    if (!P.preps.empty()) HIP_TRY(h->up.flush(h->stream));  // the prepare kernels read J on the device
    for (const DensePrep& pr : P.preps) {
        double* J = h->d_dp_data.p + pr.off;
        double* Jt = J + (size_t)pr.nf * pr.n;
        double* H = Jt + (size_t)pr.n * pr.nf;
        const long long items = (long long)pr.nf * pr.n;
        hipLaunchKernelGGL(k_dense_prior_prepare, dim3((unsigned)((items + 255) / 256)), dim3(256), 0, h->stream, J, Jt, pr.nf, pr.n);
        if (h->dprior_per_win[pr.w].resident && h->prior.hg_valid && h->prior.n == pr.n)
            hipLaunchKernelGGL(k_sym_from_lower, dim3((unsigned)(((long long)pr.n * pr.n + 255) / 256)), dim3(256), 0, h->stream, h->prior.H.p, pr.n, H);   // H = Ak of the marginalisation
        else
            hipLaunchKernelGGL(k_mgemm, dim3((pr.n + 63) / 64, (pr.n + 63) / 64), dim3(256), 0, h->stream, H, (long long)pr.n, J, 1LL, (long long)pr.n, J, (long long)pr.n, 1LL,
                               pr.n, pr.n, pr.nf, 1.0, 0.0);
    }
    if (h->env.debug & 8192) {   // the plan's scalars, for scripts/layout_same_uploads.py
        int hb_sum = 0, hb_max = 0;
        for (const HostWin& H : P.wins) { hb_sum += H.hb_lmk; hb_max = std::max(hb_max, H.hb_lmk); }
        fprintf(stderr, "[sadvio dbg] layout scalars tiles %zu max_tile_kf %d max_tile_free %d max_gemm_free %d gemm_run4 %d lm_ok %d lm_landmarks %lld lm_sub_obs %d lm_ksub %d "
                "lm_max_cam %d lm_n_sub %d max_n_kf %d max_npose %d max_np %d n_big %d hb_lmk %d/%d pre_ok %d totals %d %d %d %d reduced %d %lld %lld dp_total %lld\n",
                P.tiles.size(), P.max_tile_kf, P.max_tile_free, P.max_gemm_free, (int)P.gemm_run4, (int)P.lm_ok, P.lm_landmarks, P.lm_sub_obs, P.lm_ksub, P.lm_max_cam, P.lm_n_sub,
                P.max_n_kf, P.max_npose, P.max_np, P.n_big, hb_sum, hb_max, (int)P.pre_ok, P.n_kf_tot, P.n_cam_tot, P.n_lmk_tot, P.n_obs_tot, P.np_tot, P.s_tot, P.red_total, P.dp_total);
    }
    return SADVIO_OK;
}

// Re-plan the reduced systems and put them on the device: called by the setters of factors that hold landmarks or lines in the reduced
// system (the landmark tiles are unchanged)
int layout_reduced(sadvio_ba_handle* h) {
    const int rc = layout_reduced_plan(layout_inputs(h), h->plan, h->err);
    return rc != SADVIO_OK ? rc : layout_reduced_device(h);
}

int upload_priors(sadvio_ba_handle* h) {
    std::vector<HostWin>& wins = h->plan.wins;
    h->priors.clear();
    for (size_t w = 0; w < wins.size(); w++) {
        wins[w].d.prior_begin = (int)h->priors.size();
        for (auto& p : h->priors_per_win[w]) h->priors.push_back(p);
        wins[w].d.prior_end = (int)h->priors.size();
    }
    HIP_TRY(h->d_priors.alloc(h->priors.size()));
    HIP_TRY(h->d_prior_lin.alloc(2 * h->priors.size() * (size_t)PRIOR_LIN));
    if (!h->priors.empty())
        h->up.add(h->d_priors.p, h->priors.data(), h->priors.size() * sizeof(PriorDev));
    h->imus.clear();
    for (size_t w = 0; w < wins.size(); w++) {
        wins[w].d.imu_begin = (int)h->imus.size();
        for (auto& f : h->imus_per_win[w]) { h->imus.push_back(f); h->imus.back().win = (int)w; }
        wins[w].d.imu_end = (int)h->imus.size();
    }
    HIP_TRY(h->d_imus.alloc(h->imus.size()));
    HIP_TRY(h->d_imu_scratch.alloc(2 * h->imus.size() * (size_t)IMU_ROW));
    if (!h->imus.empty())
        h->up.add(h->d_imus.p, h->imus.data(), h->imus.size() * sizeof(ImuDev));
    std::vector<WinDev> wd(wins.size());
    for (size_t w = 0; w < wins.size(); w++) wd[w] = wins[w].d;
    h->up.add(h->d_win.p, wd.data(), wd.size() * sizeof(WinDev));
    HIP_TRY(h->up.flush(h->stream));  // one staged copy + scatter for everything queued since the layout build began
    if (h->plan.pre_ok && h->pre_dirty) {
        hipLaunchKernelGGL(k_pre_packets, dim3((unsigned)h->plan.tiles.size()), dim3(BUILD_THREADS), 0, h->stream, h->d_tiles.p, h->d_lmk_ob.p, h->d_lmk_oe.p, h->d_tile_kf.p,
                           h->d_tile_lmk.p, h->d_kf_fidx.p, (int4*)h->d_pre_lane.p, (int2*)h->d_pre_kf.p);
        h->pre_dirty = false;
    }
    return SADVIO_OK;
}

// (Re)build the device layout from the stored caller windows + the current factor lists: plan it (layout_plan.h), then allocate,
// queue and flush. A failed build leaves h->uploaded false.
int layout_build(sadvio_ba_handle* h) {
    const bool dbg_t = (h->env.debug & 8192) != 0;
    auto t_start = std::chrono::steady_clock::now();
    auto lap = [&](const char* what) { if (dbg_t) { auto t = std::chrono::steady_clock::now(); fprintf(stderr, "[sadvio dbg] build_layout %-14s %.3f ms\n", what, std::chrono::duration<double, std::milli>(t - t_start).count()); t_start = t; } };
    HIP_TRY(hipSetDevice(h->device));
    h->uploaded = false; h->solved = false;
    h->up.reset();
    LayoutPlan& P = h->plan;
    int rc = layout_plan(layout_inputs(h), P, h->err, lap);
    if (rc != SADVIO_OK) return rc;
    const size_t kf_b = P.n_kf_tot, lmk_b = std::max(P.n_lmk_tot, 1), n_tiles = P.tiles.size();
    if (h->env.debug) {
        auto chunks = [&](int ti) { return P.tiles[ti].chunk1 - P.tiles[ti].chunk0; };
        if (P.want_lm && n_tiles)
            fprintf(stderr, "[sadvio dbg] chunks per tile: largest %d, median %d, smallest %d\n", chunks(P.perm.front()), chunks(P.perm[n_tiles / 2]), chunks(P.perm.back()));
        int hist[32] = {0}, modes[3] = {0};
        for (auto& t : P.tiles) { hist[std::min(t.n_free, 31)]++; modes[t.lds_mode]++; }
        fprintf(stderr, "[sadvio dbg] %zu tiles, modes global/atomic/gemm = %d/%d/%d, max_tile_kf %d, n_free histogram:", n_tiles, modes[0], modes[1], modes[2], P.max_tile_kf);
        for (int i = 0; i < 32; i++) if (hist[i]) fprintf(stderr, " %d:%d", i, hist[i]);
        fprintf(stderr, "\n");
    }
    if (P.want_lm) {
        HIP_TRY(h->d_lm_hg.alloc(2 * (size_t)LM_HG * lmk_b));
        const size_t n_rec = std::max<size_t>(n_tiles, 1) * P.lm_ksub;
        HIP_TRY(h->d_lm_dt.alloc(2 * (size_t)LM_DT * n_rec));
        HIP_TRY(h->d_lm_sacc.alloc(2 * 4 * n_rec));
        HIP_TRY(hipMemsetAsync(h->d_lm_sacc.p, 0, sizeof(double) * 2 * 4 * n_rec, h->stream));   // slots of sub-blocks that do not exist stay zero
        // k_build_obs sums a tile's key-frame record over EVERY sub-block slot, k_lm_pass writes one slot per work item: the slots
        // nobody writes must be zero, and the buffer is grow-only (a re-layout with another tiling would leave stale records there)
        HIP_TRY(hipMemsetAsync(h->d_lm_dt.p, 0, sizeof(double) * 2 * (size_t)LM_DT * n_rec, h->stream));
    }
    HIP_TRY(h->d_chunk_ob.alloc(P.chunk_ob.size())); HIP_TRY(h->d_chunk_lm.alloc(P.chunk_lm.size())); HIP_TRY(h->d_obs_lslot.alloc(P.obs_lslot.size()));
    HIP_TRY(h->d_tile_perm.alloc(std::max<size_t>(P.perm.size(), 1))); HIP_TRY(h->d_lm_sub.alloc(std::max<size_t>(P.sub.size(), 2)));
    HIP_TRY(h->d_win.alloc(P.wins.size())); HIP_TRY(h->d_tacc.alloc(2 * n_tiles));
    HIP_TRY(h->d_tile_kf.alloc(P.tile_kf.size())); HIP_TRY(h->d_tile_row.alloc(P.tile_row.size())); HIP_TRY(h->d_tile_lmk.alloc(P.tile_lmk.size()));
    HIP_TRY(h->d_obs_slot.alloc(P.obs_slot.size())); HIP_TRY(h->d_ptab.alloc(2 * (size_t)POSE_TAB * kf_b));
    HIP_TRY(h->d_kf_T0.alloc(P.kf_T0.size())); HIP_TRY(h->d_kf_fidx.alloc(P.kf_fidx.size()));
    HIP_TRY(h->d_xp.alloc(2 * 6 * kf_b)); HIP_TRY(h->d_xv.alloc(2 * 3 * kf_b));
    HIP_TRY(h->d_xba.alloc(2 * 3 * kf_b)); HIP_TRY(h->d_xbg.alloc(2 * 3 * kf_b));
    HIP_TRY(h->d_kf_vel.alloc(P.kf_vel.size())); HIP_TRY(h->d_kf_ba.alloc(P.kf_ba.size())); HIP_TRY(h->d_kf_bg.alloc(P.kf_bg.size()));
    HIP_TRY(h->d_cam_K.alloc(P.cam_K.size())); HIP_TRY(h->d_cam_T.alloc(P.cam_T.size())); HIP_TRY(h->d_cam_isig.alloc(P.cam_isig.size()));
    HIP_TRY(h->d_lmk_p.alloc(P.lmk_p.size())); HIP_TRY(h->d_xl.alloc(2 * 3 * lmk_b));
    HIP_TRY(h->d_s_lmk.alloc(3 * lmk_b));
    HIP_TRY(h->d_lmk_ob.alloc(P.lmk_ob.size())); HIP_TRY(h->d_lmk_oe.alloc(P.lmk_oe.size()));
    HIP_TRY(h->d_obs_kf.alloc(P.obs_kf.size())); HIP_TRY(h->d_obs_cam.alloc(P.obs_cam.size())); HIP_TRY(h->d_obs_meas.alloc(P.obs_meas.size()));
    queue_table(h, h->d_chunk_ob, P.chunk_ob); queue_table(h, h->d_chunk_lm, P.chunk_lm); queue_table(h, h->d_obs_lslot, P.obs_lslot);
    queue_table(h, h->d_tile_perm, P.perm); queue_table(h, h->d_lm_sub, P.sub);
    queue_table(h, h->d_kf_T0, P.kf_T0); queue_table(h, h->d_kf_fidx, P.kf_fidx); queue_table(h, h->d_kf_vel, P.kf_vel);
    queue_table(h, h->d_kf_ba, P.kf_ba); queue_table(h, h->d_kf_bg, P.kf_bg); queue_table(h, h->d_cam_K, P.cam_K); queue_table(h, h->d_cam_T, P.cam_T);
    queue_table(h, h->d_cam_isig, P.cam_isig); queue_table(h, h->d_lmk_p, P.lmk_p);
    queue_table(h, h->d_lmk_ob, P.lmk_ob); queue_table(h, h->d_lmk_oe, P.lmk_oe); queue_table(h, h->d_obs_kf, P.obs_kf);
    queue_table(h, h->d_obs_cam, P.obs_cam); queue_table(h, h->d_obs_meas, P.obs_meas); queue_table(h, h->d_tile_kf, P.tile_kf);
    queue_table(h, h->d_tile_row, P.tile_row); queue_table(h, h->d_tile_lmk, P.tile_lmk); queue_table(h, h->d_obs_slot, P.obs_slot);
    if (P.n_long > 0) {   // (a layout without long tracks uploads what it uploaded before)
        HIP_TRY(h->d_long_rec.alloc(P.long_rec.size())); HIP_TRY(h->d_long_kf.alloc(P.long_kf.size())); HIP_TRY(h->d_long_slot.alloc(P.long_slot.size()));
        queue_table(h, h->d_long_rec, P.long_rec); queue_table(h, h->d_long_kf, P.long_kf); queue_table(h, h->d_long_slot, P.long_slot);
    }
    // First-round packets: what a lane of k_build / k_backsub needs to address the inputs of its tile's FIRST landmark round, laid out
    // by (tile, 8-lane granule) so that the loads hang on blockIdx alone: one int4 per 8 lanes, | landmark | its first observation |
    // its observation count + valid << 16 | position of the 8 lanes' first one in the landmark's group |, and per tile the first PRE_KF
    // key-frames of its list with their free index: 576 B per tile. Without them the kernel's opening is a chain tile record -> CSR
    // range / key-frame list -> observation / pose table (three dependent round trips of ~1 us each on a single window); with them
    // two. Built on the device behind the upload (k_pre_packets, upload_priors): host stores + PCIe otherwise.
    if (P.pre_ok) {
        HIP_TRY(h->d_pre_lane.alloc((size_t)4 * (BUILD_THREADS / 8) * n_tiles)); HIP_TRY(h->d_pre_kf.alloc((size_t)2 * PRE_KF * n_tiles));
        h->pre_dirty = true;
    }
    h->rel.csr_win = -1;   // the per-key-frame landmark lists of marginalize_relative_batch describe the old layout
    lap("alloc+queue");
    rc = layout_reduced_device(h);
    if (rc != SADVIO_OK) return rc;
    lap("reduced device");
    rc = upload_priors(h);  // also uploads the window descriptors
    if (rc != SADVIO_OK) return rc;
    lap("flush");
    h->uploaded = true;
    for (auto& k : h->kclasses) { k.total_ms = 0; k.launches = 0; }
    return SADVIO_OK;
}

}  // namespace
