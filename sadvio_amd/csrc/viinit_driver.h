// viinit_driver.h — the host side of sadvio_ba_vi_init: the column layout of the program, one packed allocation, one launch of
// k_viinit (viinit_kernels.h), the results unpacked. The entry point (ba_capi.hip) has checked the arguments.
// Part of the library's single translation unit (ba_capi.hip); not a public header.
#pragma once
#include "ba_handle.h"
#include "imu_host.h"
#include "solve_opts.h"

namespace {

int vi_init(sadvio_ba_handle* h, const sadvio_viinit_problem* pb, const sadvio_solve_options* opts, sadvio_solve_summary* sum, sadvio_viinit_result* res, double* dv3) {
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
        solve_opts_from(*opts, P.o);
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
        summary_from_tail(out.data() + D, S);
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

}  // namespace
