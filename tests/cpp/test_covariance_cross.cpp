// C++ check of HipOptimizer::covarianceCross and innovation_gate (include/sadvio_optimizer.hpp) on a small stereo local map solved
// through localMapBA: shapes and addressing by id, zeros for the fixed frame, the joint covariance [[Sigma_aa, Sigma_al], [Sigma_la,
// Sigma_ll]] of every candidate — Sigma_aa and Sigma_ll from covariance(), Sigma_al from covarianceCross() — positive definite,
// P = I + a positive semi-definite matrix, the gate on an exact and on a displaced measurement, refusals. The bars against the full
// inverse are the Python tests'. Exit code 0 = pass. Needs a gfx950 device.
#include <cmath>
#include <cstdio>
#include <random>
#include <vector>

#include "sadvio_optimizer.hpp"

using namespace sadvio;

static void project(const FrameState& f, int cam, const double* p, double& u, double& v) {
    const CameraModel& c = f.cameras[cam];
    double pf[3], ps[3];
    for (int i = 0; i < 3; i++) pf[i] = f.T_f_w.R[3 * i] * p[0] + f.T_f_w.R[3 * i + 1] * p[1] + f.T_f_w.R[3 * i + 2] * p[2] + f.T_f_w.t[i];
    for (int i = 0; i < 3; i++) ps[i] = c.T_s_f.R[3 * i] * pf[0] + c.T_s_f.R[3 * i + 1] * pf[1] + c.T_s_f.R[3 * i + 2] * pf[2] + c.T_s_f.t[i];
    u = c.fx * ps[0] / ps[2] + c.cx; v = c.fy * ps[1] / ps[2] + c.cy;
}

// newest first; the oldest frame carries a prior (tests/cpp/test_optimizer.cpp's map)
static LocalMapSnapshot make_map(std::mt19937& rng, int n_frames, int n_lmk) {
    std::uniform_real_distribution<double> U(-1.0, 1.0);
    LocalMapSnapshot m;
    for (int i = 0; i < n_frames; i++) {
        FrameState f;
        f.id = 100 + i;
        f.T_f_w.t[0] = -0.3 * (n_frames - 1 - i);
        CameraModel c0{458.654, 457.296, 367.215, 248.375, Pose()}, c1 = c0;
        c1.T_s_f.t[0] = -0.11;
        f.cameras = {c0, c1};
        m.frames.push_back(f);
    }
    m.frames.back().has_prior = true;
    m.frames.back().T_prior = m.frames.back().T_f_w;
    for (double& x : m.frames.back().inf_prior) x = 100.0;
    for (int l = 0; l < n_lmk; l++) {
        LandmarkState L;
        L.id = 5000 + l;
        L.p[0] = 2.0 * U(rng) + 0.3; L.p[1] = 1.2 * U(rng); L.p[2] = 4.0 + 2.0 * U(rng);
        for (int i = 0; i < n_frames; i++)
            for (int c = 0; c < 2; c++) {
                double u, v;
                project(m.frames[i], c, L.p, u, v);
                if (u > 80 && u < 650 && v > 60 && v < 430) L.features.push_back({i, c, u, v});
            }
        if ((int)L.features.size() >= 4) m.landmarks.push_back(L);
    }
    return m;
}

// Cholesky of the n x n row-major A succeeds with every pivot positive
static bool positive_definite(std::vector<double> A, int n) {
    for (int j = 0; j < n; j++) {
        double d = A[(size_t)j * n + j];
        for (int k = 0; k < j; k++) d -= A[(size_t)j * n + k] * A[(size_t)j * n + k];
        if (!(d > 0.0)) return false;
        const double l = std::sqrt(d);
        A[(size_t)j * n + j] = l;
        for (int i = j + 1; i < n; i++) {
            double v = A[(size_t)i * n + j];
            for (int k = 0; k < j; k++) v -= A[(size_t)i * n + k] * A[(size_t)j * n + k];
            A[(size_t)i * n + j] = v / l;
        }
    }
    return true;
}

int main() {
    std::mt19937 rng(20261020);
    std::normal_distribution<double> G(0.0, 1.0);
    int fails = 0;
    auto check = [&](bool ok, const char* what) { std::printf("%-100s %s\n", what, ok ? "ok" : "FAIL"); if (!ok) fails++; };

    check(innovation_gate(0.0) && innovation_gate(5.99) && !innovation_gate(6.0) && !innovation_gate(std::nan("")) && !innovation_gate(-1.0),
          "innovation_gate: 95 % of chi-square with two degrees of freedom, NaN never passes");
    check(innovation_gate(3.84, 1) && !innovation_gate(3.85, 1) && innovation_gate(7.81, 3) && !innovation_gate(7.82, 3) && !innovation_gate(1.0, 4),
          "innovation_gate: one and three degrees of freedom; an unknown dof never passes");

    HipOptimizer opt(0);
    std::vector<double> xc;
    check(!opt.covarianceCross({100}, {5000}, nullptr, nullptr, &xc, nullptr, nullptr) && !opt.last_error().empty(), "before a solve: refused");

    LocalMapSnapshot truth = make_map(rng, 4, 120), m = truth;
    for (size_t i = 0; i + 1 < m.frames.size(); i++) {
        double d[6] = {0.01 * G(rng), 0.01 * G(rng), 0.01 * G(rng), 0.03 * G(rng), 0.03 * G(rng), 0.03 * G(rng)};
        apply_pose_delta(m.frames[i].T_f_w, d);
    }
    for (auto& L : m.landmarks) for (double& x : L.p) x += 0.05 * G(rng);
    for (int rep = 0; rep < 3; rep++) check(opt.localMapBA(m, 1), "localMapBA returns true");

    // every landmark with the newest frame, then with the fixed oldest one; camera 0; the measurement the solved state predicts
    const size_t nl = m.landmarks.size(), n = 2 * nl;
    std::vector<int64_t> fid, lid, lids;
    std::vector<int32_t> cams(n, 0);
    std::vector<double> meas;
    for (size_t i = 0; i < n; i++) {
        const FrameState& f = i < nl ? m.frames.front() : m.frames.back();
        const LandmarkState& L = m.landmarks[i % nl];
        fid.push_back(f.id); lid.push_back(L.id);
        if (i < nl) lids.push_back(L.id);
        double u, v;
        project(f, 0, L.p, u, v);
        meas.push_back(u); meas.push_back(v);
    }
    std::vector<double> pc, m2, kc, lc;
    std::vector<int32_t> st;
    check(opt.covarianceCross(fid, lid, &cams, &meas, &xc, &pc, &m2, &st), "covarianceCross returns true");
    std::printf("   last_error: '%s'\n", opt.last_error().c_str());
    const int d = opt.block_dim();
    check(d == 6 && xc.size() == 3 * (size_t)d * n && pc.size() == 4 * n && m2.size() == n && st.size() == n, "output shapes");
    check(opt.covariance({m.frames.front().id}, {}, lids, &kc, nullptr, &lc), "covariance of the newest frame and every landmark");
    bool zero_fixed = true, nonzero_free = true, joint_pd = true, p_ok = true, gate_exact = true;
    int n_ok = 0;
    for (size_t i = 0; i < n; i++) {
        const double* X = &xc[18 * i];
        double mx = 0.0;
        for (int q = 0; q < 18; q++) mx = std::fmax(mx, std::fabs(X[q]));
        if (i >= nl) { zero_fixed &= mx == 0.0; continue; }
        nonzero_free &= mx > 0.0;
        std::vector<double> J(81);
        for (int a = 0; a < 6; a++) for (int b = 0; b < 6; b++) J[9 * a + b] = kc[6 * a + b];
        for (int a = 0; a < 6; a++) for (int j = 0; j < 3; j++) { J[9 * a + 6 + j] = X[3 * a + j]; J[9 * (6 + j) + a] = X[3 * a + j]; }
        for (int a = 0; a < 3; a++) for (int j = 0; j < 3; j++) J[9 * (6 + a) + 6 + j] = lc[9 * i + 3 * a + j];
        joint_pd &= positive_definite(J, 9);
        if (st[i] != SADVIO_CROSS_OK) continue;
        n_ok++;
        const double* P = &pc[4 * i];
        p_ok &= P[0] >= 1.0 && P[3] >= 1.0 && P[1] == P[2] && (P[0] - 1.0) * (P[3] - 1.0) >= P[1] * P[1] * (1.0 - 1e-12);
        gate_exact &= m2[i] < 1e-12 && innovation_gate(m2[i]);
    }
    check(zero_fixed, "the fixed oldest frame: every cross block is zero");
    check(nonzero_free, "the newest frame: no cross block is zero");
    check(joint_pd, "[[Sigma_aa, Sigma_al], [Sigma_la, Sigma_ll]] of every candidate is positive definite");
    check(n_ok > (int)nl / 2 && p_ok, "P - I is symmetric positive semi-definite");
    check(gate_exact, "the predicted measurement itself: maha2 = 0, inside the gate");
    // a measurement 400 px off is outside the gate
    {
        std::vector<double> far = meas;
        for (size_t i = 0; i < n; i++) far[2 * i] += 400.0;
        std::vector<double> m2f;
        check(opt.covarianceCross(fid, lid, &cams, &far, nullptr, nullptr, &m2f), "covarianceCross with maha2 alone");
        bool out = true;
        for (size_t i = 0; i < nl; i++)
            if (st[i] == SADVIO_CROSS_OK) out &= m2f[i] > 0.0 && !innovation_gate(m2f[i]);
        check(out, "400 px off: outside the gate");
    }
    // cross blocks only; repeats; the same bits
    {
        std::vector<double> x2;
        std::vector<int32_t> s2;
        check(opt.covarianceCross({fid[5], fid[0], fid[5]}, {lid[5], lid[0], lid[5]}, nullptr, nullptr, &x2, nullptr, nullptr, &s2) && x2.size() == 54,
              "cross blocks only, with a repeat");
        bool same = x2.size() == 54;
        for (int q = 0; q < 18 && same; q++) same &= x2[q] == xc[18 * 5 + q] && x2[36 + q] == xc[18 * 5 + q] && x2[18 + q] == xc[q];
        check(same, "a candidate's bits depend neither on its position nor on the other candidates");
    }
    check(!opt.covarianceCross({999}, {lid[0]}, nullptr, nullptr, &xc, nullptr, nullptr), "an unknown frame id: refused");
    check(!opt.covarianceCross({fid[0]}, {lid[0]}, nullptr, nullptr, nullptr, &pc, nullptr), "innov_cov without cams: refused by the library");
    {
        std::vector<int32_t> c2{2};
        std::vector<double> uv{0.0, 0.0};
        check(!opt.covarianceCross({fid[0]}, {lid[0]}, &c2, &uv, nullptr, &pc, nullptr), "a camera the frame does not have: refused");
    }
    std::printf(fails ? "FAILED (%d)\n" : "PASSED\n", fails);
    return fails ? 1 : 0;
}
