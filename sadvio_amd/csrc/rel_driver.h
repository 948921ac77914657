// rel_driver.h — the host side of sadvio_ba_marginalize_relative_batch as named steps
//   rel_check -> rel_index -> rel_launch -> rel_read_back
// The kernel is rel_kernels.h's: one launch, one workgroup per pair, everything down to the 6 x 6 information on the device. The host
// checks the arguments (O(n_pair)), builds the window's per-key-frame landmark lists once per layout (O(n_obs)), uploads the pairs,
// and copies n_pair rows back behind one wait. Nothing of the solve is touched: the window's arrays are read only and the work
// buffers are the handle's RelScratch. sadvio_ba_marginalize_relative (marg_driver.h) and its kernels are not involved.
// Part of the library's single translation unit (ba_capi.hip); not a public header.
#pragma once
#include "ba_handle.h"
#include "rel_kernels.h"
#include "marg_driver.h"

namespace {

// 1. State and arguments, in the order and wording of sadvio_ba_marginalize_relative. Host work only; nothing is written on an error.
int rel_check(sadvio_ba_handle* h, int w, int n_pair, const int32_t* kf_a, const int32_t* kf_b, int eig_cut_mode, const double* inf36, const int32_t* status) {
    if (int rc = entry_state(h, "marginalize_relative_batch", NEED_UPLOADED | NOT_DEFERRED)) return rc;
    if (w < 0 || w >= (int)h->plan.wins.size()) { h->err = "marginalize_relative_batch: window out of range"; return SADVIO_E_INVALID_ARG; }
    if (eig_cut_mode != SADVIO_EIG_CUT_REFERENCE && eig_cut_mode != SADVIO_EIG_CUT_NOISE_FLOOR) { h->err = "marginalize_relative_batch: bad eig_cut_mode"; return SADVIO_E_INVALID_ARG; }
    if (h->world > 1) { h->err = "marginalize_relative_batch: the window is sharded over several GPUs (each rank holds a landmark partition only)"; return SADVIO_E_INVALID_ARG; }
    const WinDev& d = h->plan.wins[w].d;
    if (d.has_imu) { h->err = "marginalize_relative_batch: frames with IMU states are not supported (the reference's own column layout for them is inconsistent, BundleAdjustmentCERESAnalytic.cpp:705-737)"; return SADVIO_E_INVALID_ARG; }
    if (n_pair < 0) { h->err = "marginalize_relative_batch: negative pair count"; return SADVIO_E_INVALID_ARG; }
    if (n_pair == 0) return SADVIO_OK;
    if (!kf_a || !kf_b || !inf36 || !status) { h->err = "marginalize_relative_batch: null kf_a / kf_b / inf36 / status"; return SADVIO_E_INVALID_ARG; }
    for (int i = 0; i < n_pair; i++)
        if (kf_a[i] < 0 || kf_a[i] >= d.n_kf || kf_b[i] < 0 || kf_b[i] >= d.n_kf || kf_a[i] == kf_b[i]) { h->err = "marginalize_relative_batch: bad key-frame index"; return SADVIO_E_INVALID_ARG; }
    return SADVIO_OK;
}

// 2. The window's per-key-frame lists of distinct landmarks (window order; pseudo-observations of sparse prior factors skipped), once per
// layout; the pairs; the output rows. O(n_obs) the first time, O(n_pair) afterwards; no allocation once the buffers have grown.
int rel_index(sadvio_ba_handle* h, int w, int n_pair, const int32_t* kf_a, const int32_t* kf_b) {
    RelScratch& S = h->rel;
    const WinDev& d = h->plan.wins[w].d;
    if (S.csr_win != w) {
        std::vector<int>& ptr = S.h_ptr; std::vector<int>& lst = S.h_lmk; std::vector<int>& last = S.h_last;
        ptr.assign((size_t)d.n_kf + 1, 0); last.assign((size_t)d.n_kf, -1);
        auto visit = [&](bool fill) {
            for (int l = 0; l < d.n_lmk; l++) {
                const int gl = d.lmk_base + l;
                for (int o = h->plan.lmk_ob[gl]; o < h->plan.lmk_oe[gl]; o++) {
                    if (h->plan.obs_perm[o] < 0) continue;
                    const int k = h->plan.obs_kf[o] - d.kf_base;
                    if (k < 0 || k >= d.n_kf || last[k] == gl) continue;
                    last[k] = gl;
                    if (fill) lst[ptr[k]++] = gl; else ptr[k + 1]++;
                }
            }
        };
        visit(false);
        for (int k = 0; k < d.n_kf; k++) ptr[k + 1] += ptr[k];
        S.n_kf_lmk = ptr[d.n_kf];
        lst.assign((size_t)std::max(S.n_kf_lmk, 1), 0);
        std::fill(last.begin(), last.end(), -1);
        visit(true);
        for (int k = d.n_kf; k > 0; k--) ptr[k] = ptr[k - 1];   // the fill advanced every start to its end
        ptr[0] = 0;
        HIP_TRY(S.kf_ptr.alloc(ptr.size())); HIP_TRY(S.kf_lmk.alloc(lst.size()));
        HIP_TRY(hipMemcpyAsync(S.kf_ptr.p, ptr.data(), sizeof(int) * ptr.size(), hipMemcpyHostToDevice, h->stream));
        HIP_TRY(hipMemcpyAsync(S.kf_lmk.p, lst.data(), sizeof(int) * lst.size(), hipMemcpyHostToDevice, h->stream));
        S.csr_win = w;
    }
    const size_t n = (size_t)n_pair;
    HIP_TRY(S.pairs.alloc(2 * n)); HIP_TRY(S.n_shared.alloc(n)); HIP_TRY(S.status.alloc(n));
    HIP_TRY(S.inf.alloc(36 * n)); HIP_TRY(S.Ak.alloc(144 * n)); HIP_TRY(S.Tab.alloc(12 * n));
    S.h_pairs.resize(2 * n);
    for (size_t i = 0; i < n; i++) { S.h_pairs[i] = kf_a[i]; S.h_pairs[n + i] = kf_b[i]; }
    HIP_TRY(hipMemcpyAsync(S.pairs.p, S.h_pairs.data(), sizeof(int) * 2 * n, hipMemcpyHostToDevice, h->stream));
    return SADVIO_OK;
}

// 3. One launch for all pairs
int rel_launch(sadvio_ba_handle* h, int w, int n_pair, int eig_cut_mode) {
    RelScratch& S = h->rel;
    const WinDev& d = h->plan.wins[w].d;
    SolveOpts o{};
    const DevPtrs P = make_ptrs(h, o, 1);
    RelDev R{};
    R.kf_a = S.pairs.p; R.kf_b = S.pairs.p + n_pair; R.n_pair = n_pair;
    R.kf_base = d.kf_base; R.n_lmk_tot = h->plan.n_lmk_tot; R.n_obs_tot = h->plan.n_obs_tot; R.n_cam_tot = h->plan.n_cam_tot;
    R.kf_ptr = S.kf_ptr.p; R.kf_lmk = S.kf_lmk.p; R.n_kf_lmk = S.n_kf_lmk;
    R.noise_floor = eig_cut_mode == SADVIO_EIG_CUT_NOISE_FLOOR ? 1 : 0;
    R.inf = S.inf.p; R.Ak = S.Ak.p; R.Tab = S.Tab.p; R.n_shared = S.n_shared.p; R.status = S.status.p;
    ScopedTimer t(h, "k_rel_batch");
    hipLaunchKernelGGL(h->plan.factor_type == SADVIO_FACTOR_PIXEL ? k_rel_batch<0> : k_rel_batch<1>, dim3((unsigned)n_pair), dim3(REL_THREADS), 0, h->stream, P, R);
    HIP_TRY(hipGetLastError());
    return SADVIO_OK;
}

// 4. n_pair rows per output the caller asked for, one wait
int rel_read_back(sadvio_ba_handle* h, int n_pair, double* inf36, double* Ak144, double* T_a_b, int32_t* n_shared, int32_t* status) {
    RelScratch& S = h->rel;
    const size_t n = (size_t)n_pair;
    HIP_TRY(hipMemcpyAsync(inf36, S.inf.p, sizeof(double) * 36 * n, hipMemcpyDeviceToHost, h->stream));
    if (Ak144) HIP_TRY(hipMemcpyAsync(Ak144, S.Ak.p, sizeof(double) * 144 * n, hipMemcpyDeviceToHost, h->stream));
    if (T_a_b) HIP_TRY(hipMemcpyAsync(T_a_b, S.Tab.p, sizeof(double) * 12 * n, hipMemcpyDeviceToHost, h->stream));
    if (n_shared) HIP_TRY(hipMemcpyAsync(n_shared, S.n_shared.p, sizeof(int32_t) * n, hipMemcpyDeviceToHost, h->stream));
    HIP_TRY(hipMemcpyAsync(status, S.status.p, sizeof(int32_t) * n, hipMemcpyDeviceToHost, h->stream));
    HIP_TRY(hipStreamSynchronize(h->stream));
    if (h->cfg.profile_kernels) collect_timers(h);
    return SADVIO_OK;
}

int rel_run(sadvio_ba_handle* h, int w, int n_pair, const int32_t* kf_a, const int32_t* kf_b, int eig_cut_mode, double* inf36, double* Ak144, double* T_a_b,
            int32_t* n_shared, int32_t* status) {
    if (int rc = rel_check(h, w, n_pair, kf_a, kf_b, eig_cut_mode, inf36, status)) return rc;
    if (n_pair == 0) return SADVIO_OK;
    HIP_TRY(hipSetDevice(h->device));
    if (int rc = rel_index(h, w, n_pair, kf_a, kf_b)) return rc;
    if (int rc = rel_launch(h, w, n_pair, eig_cut_mode)) return rc;
    return rel_read_back(h, n_pair, inf36, Ak144, T_a_b, n_shared, status);
}

}  // namespace
