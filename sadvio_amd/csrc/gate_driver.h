// gate_driver.h — the host side of the per-window probes: sadvio_ba_linearize, sadvio_ba_landmark_chi2 and
// sadvio_ba_landmark_chi2_models. They share the kernel arguments (gate_ptrs), the upload of the caller's deltas (gate_put_deltas),
// the launch size (gate_blocks), the pixel weight (gate_isig) and the inlier rule (gate_unpack); each keeps its own upload shape:
// linearize writes the handle's delta buffers, landmark_chi2 copies its tables one by one into scratch, landmark_chi2_models stages
// everything on the host and sends one copy. The entry points (ba_capi.hip) have checked the handle's state and the window index.
// Part of the library's single translation unit (ba_capi.hip); not a public header.
#pragma once
#include "ba_handle.h"
#include "solve_driver.h"

namespace {

static_assert(CAM_PINHOLE == SADVIO_CAM_PINHOLE && CAM_FISHEYE_EQUIDISTANT == SADVIO_CAM_FISHEYE_EQUIDISTANT && CAM_FISHEYE_EQUISOLID == SADVIO_CAM_FISHEYE_EQUISOLID &&
              CAM_FISHEYE_STEREOGRAPHIC == SADVIO_CAM_FISHEYE_STEREOGRAPHIC && CAM_OMNI == SADVIO_CAM_OMNI && CAM_DOUBLE_SPHERE == SADVIO_CAM_DOUBLE_SPHERE,
              "device_math.h restates the SADVIO_CAM_* kinds");

// The kernels' view of the handle at default options; xp / xl (null: the handle's own delta buffers) are window d's deltas in
// scratch, offset because the kernels index globally
DevPtrs gate_ptrs(sadvio_ba_handle* h, const WinDev& d, double* xp = nullptr, double* xl = nullptr) {
    SolveOpts o{};
    DevPtrs P = make_ptrs(h, o, 1);
    if (xp) { P.xp = xp - 6 * (ptrdiff_t)d.kf_base; P.xl = xl - 3 * (ptrdiff_t)d.lmk_base; }
    return P;
}
// the caller's deltas of window d (null: left as they are, zero) to xp / xl on the device
int gate_put_deltas(sadvio_ba_handle* h, const WinDev& d, double* xp, double* xl, const double* pose_delta6, const double* lmk_delta3) {
    if (pose_delta6) HIP_TRY(hipMemcpyAsync(xp, pose_delta6, sizeof(double) * 6 * d.n_kf, hipMemcpyHostToDevice, h->stream));
    if (lmk_delta3 && d.n_lmk) HIP_TRY(hipMemcpyAsync(xl, lmk_delta3, sizeof(double) * 3 * d.n_lmk, hipMemcpyHostToDevice, h->stream));
    return SADVIO_OK;
}
inline int gate_blocks(int n, int threads) { return (n + threads - 1) / threads; }
// 1 / sigma of the pixel residuals; 0: the cameras' own (cam_isig)
inline double gate_isig(const sadvio_ba_handle* h, double pixel_sigma) {
    return pixel_sigma > 0.0 ? 1.0 / pixel_sigma : (h->plan.factor_type == SADVIO_FACTOR_PIXEL ? 0.0 : 1.0);
}
// out2: (average chi2, observation count) per landmark. Inlier: at least two observations and an average that is not above 2
void gate_unpack(const double* out2, int n_lmk, double* avg_chi2, int32_t* inlier) {
    for (int l = 0; l < n_lmk; l++) {
        if (avg_chi2) avg_chi2[l] = out2[2 * (size_t)l];
        if (inlier) inlier[l] = (out2[2 * (size_t)l + 1] >= 2.0 && !(out2[2 * (size_t)l] > 2.0)) ? 1 : 0;
    }
}

int linearize(sadvio_ba_handle* h, int32_t w, const double* pose_delta6, const double* lmk_delta3, double* r2, double* Jp12, double* Jl6) {
    HIP_TRY(hipSetDevice(h->device));
    const WinDev& d = h->plan.wins[w].d;
    HIP_TRY(hipMemsetAsync(h->d_xp.p, 0, sizeof(double) * h->d_xp.n, h->stream));
    HIP_TRY(hipMemsetAsync(h->d_xl.p, 0, sizeof(double) * h->d_xl.n, h->stream));
    if (int rc = gate_put_deltas(h, d, h->d_xp.p + 6 * (size_t)d.kf_base, h->d_xl.p + 3 * (size_t)d.lmk_base, pose_delta6, lmk_delta3)) return rc;
    if (d.n_obs == 0) { HIP_TRY(hipStreamSynchronize(h->stream)); return SADVIO_OK; }
    HIP_TRY(h->d_probe.alloc(20 * (size_t)d.n_obs));
    DevPtrs P = gate_ptrs(h, d);
    double* pr = h->d_probe.p; double* pj = pr + 2 * (size_t)d.n_obs; double* pl = pj + 12 * (size_t)d.n_obs;
    int blocks = gate_blocks(d.n_obs, 256);
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

int landmark_chi2(sadvio_ba_handle* h, int32_t w, const double* pose_delta6, const double* lmk_delta3, const double* image_wh, double pixel_sigma,
                  double* avg_chi2, int32_t* inlier) {
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
    if (int rc = gate_put_deltas(h, d, d_sxp, d_sxl, pose_delta6, lmk_delta3)) return rc;
    HIP_TRY(hipMemcpyAsync(d_wh + 2 * (size_t)d.cam_base, wh.data(), sizeof(double) * wh.size(), hipMemcpyHostToDevice, h->stream));
    DevPtrs P = gate_ptrs(h, d, d_sxp, d_sxl);
    const int blocks = gate_blocks(d.n_lmk, 64);
    const double isig = gate_isig(h, pixel_sigma);
    if (h->plan.factor_type == SADVIO_FACTOR_PIXEL) hipLaunchKernelGGL(k_lmk_chi2<0>, dim3(blocks), dim3(64), 0, h->stream, P, w, d_wh, isig, d_out);
    else hipLaunchKernelGGL(k_lmk_chi2<1>, dim3(blocks), dim3(64), 0, h->stream, P, w, d_wh, isig, d_out);
    HIP_TRY(hipGetLastError());
    std::vector<double> hb(2 * (size_t)d.n_lmk);
    HIP_TRY(hipMemcpyAsync(hb.data(), d_out, sizeof(double) * hb.size(), hipMemcpyDeviceToHost, h->stream));
    HIP_TRY(hipStreamSynchronize(h->stream));
    gate_unpack(hb.data(), d.n_lmk, avg_chi2, inlier);
    return SADVIO_OK;
}

int landmark_chi2_models(sadvio_ba_handle* h, int32_t w, const double* pose_delta6, const double* lmk_delta3, const sadvio_camera_model* models, const double* obs_uv,
                         double pixel_sigma, double* avg_chi2, int32_t* inlier, double* obs_chi2) {
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
    DevPtrs P = gate_ptrs(h, d, d_sxp, d_sxl);
    const double* k_wh = d_wh - 2 * (ptrdiff_t)d.cam_base;                               // the kernel indexes the camera tables globally too
    const CamModelDev* k_md = (const CamModelDev*)d_md - (ptrdiff_t)d.cam_base;
    const int blocks = gate_blocks(d.n_lmk, 64);
    const double isig = gate_isig(h, pixel_sigma);
    const double* k_uv = obs_uv ? d_uv : nullptr;
    if (h->plan.factor_type == SADVIO_FACTOR_PIXEL) hipLaunchKernelGGL(k_lmk_chi2_models<0>, dim3(blocks), dim3(64), 0, h->stream, P, w, k_wh, k_md, k_uv, isig, d_ob + n_ob, d_ob);
    else hipLaunchKernelGGL(k_lmk_chi2_models<1>, dim3(blocks), dim3(64), 0, h->stream, P, w, k_wh, k_md, k_uv, isig, d_ob + n_ob, d_ob);
    HIP_TRY(hipGetLastError());
    std::vector<double> hb(n_ob + n_out);   // obs | out
    HIP_TRY(hipMemcpyAsync(hb.data(), d_ob, sizeof(double) * hb.size(), hipMemcpyDeviceToHost, h->stream));
    HIP_TRY(hipStreamSynchronize(h->stream));
    gate_unpack(hb.data() + n_ob, d.n_lmk, avg_chi2, inlier);
    if (obs_chi2)
        for (int a = 0; a < d.n_obs; a++) {
            const int src = h->plan.obs_perm[d.obs_base + a];
            if (src >= 0) obs_chi2[src] = hb[(size_t)a];
        }
    return SADVIO_OK;
}

}  // namespace
