// C++ check of sadvio_ba_covariance_batch on the plain C ABI (include/sadvio_ba.h): two small stereo windows in one batch, window 0 with
// its oldest key-frame constant (N_p = 12: the in-LDS route), window 1 with every key-frame constant (N_p = 0). The batch is compared
// item by item with sadvio_ba_covariance: the same bits on the NONE route (and on the DENSE route, on a second handle created under
// SADVIO_COV_BATCH_LDS=0), a relative block difference of at most 1e-9 on the LDS route — a smoke bar; the Python tests hold the real
// ones. Exit code 0 = pass. Needs a gfx950 device.
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <random>
#include <vector>

#include "sadvio_ba.h"

struct Window {
    std::vector<int64_t> kf_id, lmk_id;
    std::vector<double> kf_T, cam_K, cam_T, cam_sigma, lmk_p, meas;
    std::vector<uint8_t> kf_const;
    std::vector<int32_t> ptr, obs_kf, obs_cam;
    sadvio_flat_window flat() const {
        sadvio_flat_window w;
        std::memset(&w, 0, sizeof(w));
        w.n_kf = (int32_t)kf_id.size(); w.n_cam = (int32_t)cam_sigma.size(); w.n_lmk = (int32_t)lmk_id.size(); w.n_obs = (int32_t)obs_kf.size();
        w.factor_type = SADVIO_FACTOR_PIXEL; w.has_imu = 0;
        w.kf_id = kf_id.data(); w.kf_T_f_w = kf_T.data(); w.kf_const = kf_const.data();
        w.cam_K = cam_K.data(); w.cam_T_s_f = cam_T.data(); w.cam_sigma = cam_sigma.data();
        w.lmk_id = lmk_id.data(); w.lmk_p = lmk_p.data(); w.lmk_obs_ptr = ptr.data(); w.obs_kf = obs_kf.data(); w.obs_cam = obs_cam.data();
        w.obs_meas = meas.data();
        return w;
    }
};

// n_kf stereo frames 0.3 m apart along +x looking down +z; every landmark is seen by every view it projects into
static Window make_window(int n_kf, int n_lmk, bool all_const, unsigned seed) {
    std::mt19937 rng(seed);
    std::uniform_real_distribution<double> U(-1.0, 1.0);
    Window w;
    const double K[4] = {458.654, 457.296, 367.215, 248.375};
    for (int c = 0; c < 2; c++) {
        w.cam_K.insert(w.cam_K.end(), K, K + 4);
        const double T[12] = {1, 0, 0, 0, 1, 0, 0, 0, 1, c ? -0.11 : 0.0, 0, 0};
        w.cam_T.insert(w.cam_T.end(), T, T + 12);
        w.cam_sigma.push_back(1.0);
    }
    for (int k = 0; k < n_kf; k++) {
        const double T[12] = {1, 0, 0, 0, 1, 0, 0, 0, 1, -0.3 * k, 0.01 * k, 0};
        w.kf_T.insert(w.kf_T.end(), T, T + 12);
        w.kf_id.push_back(100 + k);
        w.kf_const.push_back(all_const || k == 0 ? 1 : 0);
    }
    w.ptr.push_back(0);
    for (int l = 0; l < n_lmk; l++) {
        const double p[3] = {1.5 * U(rng) + 0.3, 1.0 * U(rng), 4.0 + 2.0 * U(rng)};
        const size_t before = w.obs_kf.size();
        for (int k = 0; k < n_kf; k++)
            for (int c = 0; c < 2; c++) {
                const double x = p[0] + w.kf_T[12 * k + 9] + (c ? -0.11 : 0.0), y = p[1] + w.kf_T[12 * k + 10], z = p[2];
                const double u = K[0] * x / z + K[2], v = K[1] * y / z + K[3];
                if (u < 20 || u > 730 || v < 20 || v > 460) continue;
                w.obs_kf.push_back(k); w.obs_cam.push_back(c);
                w.meas.push_back(u + 0.3 * U(rng)); w.meas.push_back(v + 0.3 * U(rng));
            }
        if (w.obs_kf.size() - before < 4) {   // too few views: drop the landmark
            w.obs_kf.resize(before); w.obs_cam.resize(before); w.meas.resize(2 * before);
            continue;
        }
        w.lmk_id.push_back(5000 + l);
        w.lmk_p.push_back(p[0] + 0.02 * U(rng)); w.lmk_p.push_back(p[1] + 0.02 * U(rng)); w.lmk_p.push_back(p[2] + 0.05 * U(rng));
        w.ptr.push_back((int32_t)w.obs_kf.size());
    }
    return w;
}

static double rel_diff(const double* a, const double* b, size_t n) {
    double mx = 0.0, df = 0.0;
    for (size_t i = 0; i < n; i++) { mx = std::fmax(mx, std::fabs(b[i])); df = std::fmax(df, std::fabs(a[i] - b[i])); }
    return df == 0.0 ? 0.0 : df / mx;
}

static int fails = 0;
static void check(bool ok, const char* what) { std::printf("%-100s %s\n", what, ok ? "ok" : "FAIL"); if (!ok) fails++; }

// one handle: solve both windows, the batch against the single calls. expect_lds: the route window 0 must report.
static void run(const Window& A, const Window& B, bool expect_lds) {
    sadvio_ba_config cfg;
    std::memset(&cfg, 0, sizeof(cfg));
    sadvio_ba_handle* h = nullptr;
    check(sadvio_ba_create(&cfg, &h) == SADVIO_OK && h, "create");
    if (!h) return;
    const sadvio_flat_window wins[2] = {A.flat(), B.flat()};
    check(sadvio_ba_set_windows(h, 2, wins) == SADVIO_OK, "set_windows");
    sadvio_cov_batch_item none;
    std::memset(&none, 0, sizeof(none));
    check(sadvio_ba_covariance_batch(h, 1, &none) == SADVIO_E_STATE, "before the solve: SADVIO_E_STATE");
    sadvio_solve_options o;
    sadvio_ba_default_options(&o);
    sadvio_solve_summary sum[2];
    check(sadvio_ba_solve(h, &o, sum) == SADVIO_OK, "solve");
    const int32_t kf[3] = {0, 1, 2}, pa[1] = {1}, pb[1] = {2};
    const int nA = wins[0].n_lmk, nB = wins[1].n_lmk;
    std::vector<double> kfc(3 * 36, -7.0), pc(36, -7.0), lA(9 * (size_t)nA, -7.0), lB(9 * (size_t)nB, -7.0), l2(9 * 2, -7.0);
    const int32_t pick[2] = {3, 0};
    sadvio_cov_batch_item it[3];
    std::memset(it, 0, sizeof(it));
    it[0].w = 1; it[0].rq.n_lmk = -1; it[0].lmk_cov = lB.data();
    it[1].w = 0; it[1].rq.n_kf = 3; it[1].rq.kf = kf; it[1].rq.n_pair = 1; it[1].rq.pair_a = pa; it[1].rq.pair_b = pb; it[1].rq.n_lmk = -1;
    it[1].kf_cov = kfc.data(); it[1].pair_cov = pc.data(); it[1].lmk_cov = lA.data();
    it[2].w = 0; it[2].rq.n_lmk = 2; it[2].rq.lmk = pick; it[2].lmk_cov = l2.data();
    const int rc = sadvio_ba_covariance_batch(h, 3, it);
    std::printf("   batch rc %d%s%s, routes %d %d %d\n", rc, rc ? ", last_error: " : "", rc ? sadvio_ba_last_error(h) : "", it[0].route, it[1].route, it[2].route);
    check(rc == SADVIO_OK && it[0].status == SADVIO_OK && it[1].status == SADVIO_OK && it[2].status == SADVIO_OK, "the batch call and every item: SADVIO_OK");
    check(it[0].route == SADVIO_COV_ROUTE_NONE, "window 1 (every key-frame constant): route NONE");
    check(it[1].route == (expect_lds ? SADVIO_COV_ROUTE_LDS : SADVIO_COV_ROUTE_DENSE) && it[2].route == it[1].route, expect_lds ? "window 0: route LDS" : "window 0: route DENSE");
    // the single calls
    std::vector<double> skf(3 * 36), sp(36), slA(9 * (size_t)nA), slB(9 * (size_t)nB);
    int32_t nsA = -1, nsB = -1;
    sadvio_cov_request rqA = it[1].rq, rqB = it[0].rq;
    check(sadvio_ba_covariance(h, 0, &rqA, skf.data(), sp.data(), slA.data(), &nsA) == SADVIO_OK, "single call, window 0");
    check(sadvio_ba_covariance(h, 1, &rqB, nullptr, nullptr, slB.data(), &nsB) == SADVIO_OK, "single call, window 1");
    check(std::memcmp(lB.data(), slB.data(), sizeof(double) * slB.size()) == 0 && it[0].n_lmk_singular == nsB, "NONE route: the single call's bits");
    double worst = 0.0;
    for (int k = 0; k < 3; k++) worst = std::fmax(worst, rel_diff(kfc.data() + 36 * k, skf.data() + 36 * k, 36));
    worst = std::fmax(worst, rel_diff(pc.data(), sp.data(), 36));
    for (int l = 0; l < nA; l++) worst = std::fmax(worst, rel_diff(lA.data() + 9 * l, slA.data() + 9 * l, 9));
    std::printf("   window 0: worst relative block difference batch against single %.3e\n", worst);
    if (expect_lds) check(worst <= 1e-9, "LDS route: every block within 1e-9 relative of the single call's");
    else check(std::memcmp(kfc.data(), skf.data(), sizeof(double) * skf.size()) == 0 && std::memcmp(pc.data(), sp.data(), sizeof(double) * 36) == 0 &&
               std::memcmp(lA.data(), slA.data(), sizeof(double) * slA.size()) == 0, "DENSE route: the single call's bits");
    bool zero0 = true;
    for (int k = 0; k < 36; k++) zero0 &= kfc[k] == 0.0;
    check(zero0 && kfc[36] > 0.0, "the constant key-frame's block is zero, a free one's is not");
    check(std::memcmp(l2.data(), lA.data() + 27, 72) == 0 && std::memcmp(l2.data() + 9, lA.data(), 72) == 0 && it[1].n_lmk_singular == nsA,
          "a second item on window 0 (two landmarks picked): the bits of the first item's blocks");
    // arguments
    std::vector<double> guard(36, -7.0);
    sadvio_cov_batch_item bad[2];
    std::memset(bad, 0, sizeof(bad));
    const int32_t kbad[1] = {3};
    bad[0].w = 0; bad[0].rq.n_kf = 1; bad[0].rq.kf = kf; bad[0].kf_cov = guard.data();
    bad[1].w = 0; bad[1].rq.n_kf = 1; bad[1].rq.kf = kbad; bad[1].kf_cov = guard.data();
    bool untouched = sadvio_ba_covariance_batch(h, 2, bad) == SADVIO_E_INVALID_ARG;
    for (double v : guard) untouched &= v == -7.0;
    check(untouched, "a key-frame out of range in the last item: SADVIO_E_INVALID_ARG, the first item's output untouched");
    bad[1].w = 2; bad[1].rq.kf = kf;
    check(sadvio_ba_covariance_batch(h, 2, bad) == SADVIO_E_INVALID_ARG, "a window out of range: SADVIO_E_INVALID_ARG");
    check(sadvio_ba_covariance_batch(h, -1, bad) == SADVIO_E_INVALID_ARG && sadvio_ba_covariance_batch(h, 1, nullptr) == SADVIO_E_INVALID_ARG, "n_item < 0, null items: SADVIO_E_INVALID_ARG");
    check(sadvio_ba_covariance_batch(h, 0, nullptr) == SADVIO_OK, "n_item = 0: SADVIO_OK");
    sadvio_ba_destroy(h);
}

int main() {
    const Window A = make_window(3, 60, false, 20261018u), B = make_window(3, 40, true, 7u);
    std::printf("window 0: %zu landmarks, %zu observations; window 1: %zu landmarks\n", A.lmk_id.size(), A.obs_kf.size(), B.lmk_id.size());
    run(A, B, true);
    setenv("SADVIO_COV_BATCH_LDS", "0", 1);   // read when a handle is created
    run(A, B, false);
    std::printf(fails ? "FAILED (%d)\n" : "PASSED\n", fails);
    return fails ? 1 : 0;
}
