// cov_cross_driver.h — the host side of sadvio_ba_covariance_cross as named steps
//   covx_check -> cov_routes -> cov_assemble -> cov_invert -> cov_landmarks -> covx_cross (one wait)
// The steps up to cov_landmarks are cov_driver.h's (cov_landmarks for every landmark when innovation outputs are asked for, not at
// all otherwise): covx_run hands covx_cross to cov_steps as the last step, in cov_read_back's place behind the call's single wait
// (it adds none on the dense route), and so takes the single call's choice of assembly (SADVIO_COV_SQRT) and its retry.
// Dense route: k_cov_cross / k_cov_innov read block rows of Sigma_pp. Band route: k_cov_band_rows first solves the whole block row of
// every distinct key-frame asked for, and every candidate is served from those rows; no kernel reads Sigma outside its band.
// Part of the library's single translation unit (ba_capi.hip); not a public header.
#pragma once
#include "cov_cross_kernels.h"
#include "cov_cross_plan.h"
#include "cov_driver.h"

namespace {

struct CovCrossOut { double* cross; double* innov; double* maha2; int32_t* status; };

// 1. State and arguments: cov_check's refusals with its texts, then the candidates. Host work only.
int covx_check(sadvio_ba_handle* h, int w, const sadvio_cov_cross_request* rq, const CovCrossOut& O) {
    const sadvio_cov_request none{0, nullptr, 0, nullptr, nullptr, 0, nullptr};
    if (int rc = cov_check(h, w, rq ? &none : nullptr, false)) return rc;   // (the border route has no block rows yet: such a window keeps its refusal)
    const WinDev& d = h->plan.wins[w].d;
    if (rq->n < 0 || (rq->n > 0 && (!rq->kf || !rq->lmk)) || ((rq->cam == nullptr) != (rq->meas == nullptr))) { h->err = "covariance: request out of range"; return SADVIO_E_INVALID_ARG; }
    if ((O.innov || O.maha2) && !rq->cam) { h->err = "covariance_cross: innovation outputs without a candidate camera and measurement"; return SADVIO_E_INVALID_ARG; }
    const int n_cam = h->src[w].v.n_cam;   // the caller's camera count
    for (int i = 0; i < rq->n; i++) {
        if (rq->kf[i] < 0 || rq->kf[i] >= d.n_kf) { h->err = "covariance: key-frame index out of range"; return SADVIO_E_INVALID_ARG; }
        if (rq->lmk[i] < 0 || rq->lmk[i] >= d.n_lmk) { h->err = "covariance: landmark index out of range"; return SADVIO_E_INVALID_ARG; }
        if (rq->cam && (rq->cam[i] < 0 || rq->cam[i] >= n_cam)) { h->err = "covariance_cross: camera index out of range"; return SADVIO_E_INVALID_ARG; }
    }
    return SADVIO_OK;
}

// 5. The cross step: plan, upload, (band route: block rows,) cross blocks, innovations; one wait; the caller's arrays are written
// only after the pivot flag of the band route has been read.
int covx_cross(sadvio_ba_handle* h, int w, const sadvio_cov_cross_request* rq, const CovRoutes& R, const CovCrossOut& O) {
    const WinDev& d = h->plan.wins[w].d;
    CovScratch& V = h->cv;
    CovCrossScratch& K = h->cx;
    const int n = rq->n, D = d.dpf, Np = R.Np;
    const bool innov = rq->cam != nullptr;
    const int ms = R.pix ? 2 : 3;
    CovCrossPlan plan;
    cov_cross_plan(n, rq->kf, d.n_kf, h->plan.kf_fidx.data() + d.kf_base, covx_per_wg(D), plan);
    const int n_wg = plan.n_wg(), n_rows = (int)plan.rows.size();
    // one int upload: order | wgs | kf | lmk | cam | crow | first column of each block row
    std::vector<int>& I = K.h_ints;
    const size_t o_order = 0, o_wgs = (size_t)n, o_kf = o_wgs + 4 * (size_t)n_wg, o_lmk = o_kf + n, o_cam = o_lmk + n, o_crow = o_cam + n, o_col = o_crow + n;
    I.assign(o_col + (size_t)std::max(n_rows, 1), 0);
    std::copy(plan.order.begin(), plan.order.end(), I.begin() + o_order);
    std::copy(plan.wgs.begin(), plan.wgs.end(), I.begin() + o_wgs);
    std::vector<int> slot_of(d.n_free_kf > 0 ? d.n_free_kf : 0, -1);
    for (int r = 0; r < n_rows; r++) { slot_of[plan.rows[r]] = r; I[o_col + r] = plan.rows[r] * D; }
    const SrcWin& S = h->src[w];
    for (int c = 0; c < n; c++) {
        const int f = h->plan.kf_fidx[d.kf_base + rq->kf[c]];
        I[o_kf + c] = rq->kf[c]; I[o_lmk + c] = rq->lmk[c];
        I[o_cam + c] = innov ? d.cam_base + S.cam_map[rq->cam[c]] : 0;
        I[o_crow + c] = f < 0 ? -1 : (R.band ? slot_of[f] : f);
    }
    const size_t n_cross = (size_t)n * D * 3, n_out = n_cross + 5 * (size_t)n;
    HIP_TRY(K.ints.alloc(I.size())); HIP_TRY(K.status.alloc((size_t)n)); HIP_TRY(K.out.alloc(n_out));
    HIP_TRY(hipMemcpyAsync(K.ints.p, I.data(), sizeof(int) * I.size(), hipMemcpyHostToDevice, h->stream));
    if (innov) {
        HIP_TRY(K.meas.alloc((size_t)ms * n));
        HIP_TRY(hipMemcpyAsync(K.meas.p, rq->meas, sizeof(double) * (size_t)ms * n, hipMemcpyHostToDevice, h->stream));
    }
    SolveOpts so{};
    const DevPtrs P = make_ptrs(h, so, h->last_slots + 2);
    const CovDev C = cov_dev(h, w, R);
    CovCrossDev X{};
    X.n = n; X.band = R.band ? 1 : 0;
    X.stage_max = h->env.cov_cross_stage >= 0 ? std::min(h->env.cov_cross_stage, COVX_STAGE_MAX) : COVX_STAGE_MAX;
    X.rows = V.Sig.p; X.flag = nullptr;
    X.order = K.ints.p + o_order; X.wgs = K.ints.p + o_wgs; X.kf = K.ints.p + o_kf; X.lmk = K.ints.p + o_lmk; X.cam = K.ints.p + o_cam; X.crow = K.ints.p + o_crow;
    X.meas = K.meas.p; X.cross = K.out.p; X.innov = K.out.p + n_cross; X.maha2 = X.innov + 4 * (size_t)n; X.status = K.status.p;
    if (R.band) {
        X.flag = V.bflag.p;
        if (n_rows > 0) {
            HIP_TRY(K.rows.alloc((size_t)n_rows * D * Np));
            const CovBand B = cov_band_dev(h, R);
            ScopedTimer t(h, "cov_band_rows");
            hipLaunchKernelGGL(k_cov_band_rows, dim3(n_rows), dim3(COVBAND_THREADS), 0, h->stream, B, (const int*)(K.ints.p + o_col), K.rows.p);
        }
        X.rows = K.rows.p;
    }
    {
        const size_t lds = (size_t)D * Np <= (size_t)X.stage_max ? sizeof(double) * (size_t)D * Np : 0;
        auto kx = D == 6 ? (R.sqrt ? k_cov_cross<6, true> : k_cov_cross<6, false>) : (R.sqrt ? k_cov_cross<15, true> : k_cov_cross<15, false>);
        HIP_TRY(hipFuncSetAttribute((const void*)kx, hipFuncAttributeMaxDynamicSharedMemorySize, (int)(sizeof(double) * COVX_STAGE_MAX)));
        ScopedTimer t(h, "cov_cross");
        hipLaunchKernelGGL(kx, dim3(n_wg), dim3(COVX_THREADS), lds, h->stream, P, C, X);
        if (innov) {
            auto ki = D == 6 ? (R.pix ? k_cov_innov<0, 6> : k_cov_innov<1, 6>) : (R.pix ? k_cov_innov<0, 15> : k_cov_innov<1, 15>);
            hipLaunchKernelGGL(ki, dim3((n + COVX_THREADS - 1) / COVX_THREADS), dim3(COVX_THREADS), 0, h->stream, P, C, X);
        }
    }
    HIP_TRY(hipGetLastError());
    K.h_out.resize(n_out); K.h_status.resize((size_t)n);
    HIP_TRY(hipMemcpyAsync(K.h_out.data(), K.out.p, sizeof(double) * (innov ? n_out : n_cross), hipMemcpyDeviceToHost, h->stream));
    HIP_TRY(hipMemcpyAsync(K.h_status.data(), K.status.p, sizeof(int) * (size_t)n, hipMemcpyDeviceToHost, h->stream));
    int flag[2] = {0, 0};
    if (R.band) HIP_TRY(hipMemcpyAsync(flag, V.bflag.p, sizeof(flag), hipMemcpyDeviceToHost, h->stream));
    if (int rc = cov_wait(h)) return rc;
    if (flag[0] != 0) return cov_not_usable(h, true);
    if (O.cross) memcpy(O.cross, K.h_out.data(), sizeof(double) * n_cross);
    if (O.innov) memcpy(O.innov, K.h_out.data() + n_cross, sizeof(double) * 4 * (size_t)n);
    if (O.maha2) memcpy(O.maha2, K.h_out.data() + n_cross + 4 * (size_t)n, sizeof(double) * (size_t)n);
    if (O.status) for (int c = 0; c < n; c++) O.status[c] = K.h_status[c];
    return SADVIO_OK;
}

int covx_run(sadvio_ba_handle* h, int w, const sadvio_cov_cross_request* rq, double* cross_cov, double* innov_cov, double* maha2, int32_t* status) {
    const CovCrossOut O{cross_cov, innov_cov, maha2, status};
    if (int rc = covx_check(h, w, rq, O)) return rc;
    if (rq->n == 0) return SADVIO_OK;
    HIP_TRY(hipSetDevice(h->device));
    // Sigma_ll of every landmark is needed exactly when an innovation is formed
    static const double want_lmk = 0.0;
    const sadvio_cov_request all{0, nullptr, 0, nullptr, nullptr, -1, nullptr};
    return cov_steps(h, w, cov_routes(h, w, &all, rq->cam ? &want_lmk : nullptr, false), [=](const CovRoutes& R) { return covx_cross(h, w, rq, R, O); });
}

}  // namespace
