// nofov_driver.h — the host side of sadvio_ba_nofov_scale (landmarkOptimizationNoFov, AngularAdjustmentCERESAnalytic.cpp:741-907):
// validation and the constant tables on the host (nofov_plan.h), the whole LM solve and the gate in one launch of k_nofov
// (nofov_kernels.h), the results unpacked.
// Part of the library's single translation unit (ba_capi.hip); not a public header.
#pragma once
#include "ba_handle.h"
#include "nofov_plan.h"
#include "solve_opts.h"

namespace {

static_assert(NOFOV_PLAN_FTAB == NOFOV_FTAB && NOFOV_PLAN_CTAB == NOFOV_CTAB && NOFOV_PLAN_MAX_LMK == NOFOV_MAX_LMK && NOFOV_PLAN_MAX_OBS_PER_LMK == NOFOV_MAX_OBS_PER_LMK,
              "nofov_plan.h restates the sizes of nofov_kernels.h");

int nofov_scale(sadvio_ba_handle* h, const sadvio_nofov_problem* pb, const sadvio_solve_options* opts, sadvio_solve_summary* sum, sadvio_nofov_result* res,
                double* lmk_delta3, double* gate_norm, int32_t* inlier) {
    int fixed = 0;
    if (const char* why = nofov_check(pb, opts, fixed)) { h->err = why; return SADVIO_E_INVALID_ARG; }
    const int n = pb->n_lmk, no = pb->n_obs, nfr = pb->n_frames, nc = pb->n_cam;
    HIP_TRY(hipSetDevice(h->device));
    std::vector<double> ftab(NOFOV_FTAB * (size_t)nfr), ctab(NOFOV_CTAB * (size_t)nc);
    nofov_tables(pb, ftab.data(), ctab.data());
    NoFovDev P{};
    P.n_lmk = n; P.fixed = fixed; P.info = pb->info_scale; P.gate = pb->gate; P.huber_a = opts->huber_a;
    solve_opts_from(*opts, P.o);
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
    summary_from_tail(s, S);
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

}  // namespace
