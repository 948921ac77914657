// Stand-alone check of sadvio_amd/csrc/nofov_plan.h (host only; built and run by tests/test_capi_host_cpu.py):
//   the fix_scale = -1 decision on both sides of the rotation threshold (0.05 rad) and of the translation threshold (0.01), and at the
//   identity rotation (the guard on sin);
//   every refusal text of nofov_check, each from a problem in which only that condition fails.
// The constant tables are printed by dump_nofov_tables.cpp and compared in Python.
#include <cmath>
#include <cstdio>
#include <cstring>
#include <string>
#include <vector>

#include "../../sadvio_amd/csrc/nofov_plan.h"

static int fails = 0;
#define CHECK(cond, ...) do { if (!(cond)) { fails++; printf("MISMATCH %s:%d: ", __FILE__, __LINE__); printf(__VA_ARGS__); printf("\n"); } } while (0)

static void motion(double angle, double t_norm, double* T) {   // rotation about z | translation along (0.6, 0, 0.8)
    const double c = std::cos(angle), s = std::sin(angle);
    const double R[9] = {c, -s, 0, s, c, 0, 0, 0, 1};
    memcpy(T, R, sizeof(R));
    T[9] = 0.6 * t_norm; T[10] = 0.0; T[11] = 0.8 * t_norm;
}

// a problem nofov_check accepts: 2 landmarks, 3 angular factors, 2 frames, 2 cameras
struct Problem {
    std::vector<double> frames, cams, lmk_p, sbear, obear;
    std::vector<int32_t> scam, optr, ofr, ocam;
    double Tm[12];
    sadvio_nofov_problem pb;
    sadvio_solve_options opts;
    Problem() : frames(24, 0.0), cams(24, 0.0), lmk_p(6, 1.0), sbear(6, 0.5), obear(9, 0.5), scam{1, 0}, optr{0, 2, 3}, ofr{0, 1, 1}, ocam{0, 1, 0} {
        for (int k = 0; k < 2; k++) frames[12 * k] = frames[12 * k + 4] = frames[12 * k + 8] = cams[12 * k] = cams[12 * k + 4] = cams[12 * k + 8] = 1.0;
        motion(0.2, 1.0, Tm);
        memset(&pb, 0, sizeof(pb));
        memset(&opts, 0, sizeof(opts));
        pb.n_lmk = 2; pb.n_obs = 3; pb.n_frames = 2; pb.n_cam = 2; pb.cam0 = 0; pb.fix_scale = 0;
        pb.frame_T_f_w = frames.data(); pb.cam_T_s_f = cams.data(); pb.T_cam0_cam0p = Tm; pb.info_scale = 1.0; pb.gate = 0.01;
        pb.lmk_p = lmk_p.data(); pb.scale_bearing = sbear.data(); pb.scale_cam = scam.data(); pb.lmk_obs_ptr = optr.data();
        pb.obs_frame = ofr.data(); pb.obs_cam = ocam.data(); pb.obs_bearing = obear.data();
    }
};

static void refused(const char* want, const Problem& P) {
    int fixed = -7;
    const char* got = nofov_check(&P.pb, &P.opts, fixed);
    CHECK(got && std::string(got) == want, "wanted \"%s\", got \"%s\"", want, got ? got : "(accepted)");
}

int main() {
    // the decision
    struct { double angle, t; int fixed; } D[] = {{0.049, 1.0, 1}, {0.051, 1.0, 0}, {0.2, 0.009, 1}, {0.2, 0.011, 0}, {0.0, 1.0, 1}, {0.0, 0.0, 1}};
    for (const auto& d : D) {
        double T[12];
        motion(d.angle, d.t, T);
        CHECK(nofov_reference_fix_scale(T) == d.fixed, "rotation %g, translation %g: fixed = %d", d.angle, d.t, nofov_reference_fix_scale(T));
    }
    {   // through nofov_check: -1 takes the rule, 0 and 1 are the caller's
        Problem P;
        int fixed = -7;
        CHECK(!nofov_check(&P.pb, &P.opts, fixed) && fixed == 0, "fix_scale = 0: fixed = %d", fixed);
        P.pb.fix_scale = 1;
        CHECK(!nofov_check(&P.pb, &P.opts, fixed) && fixed == 1, "fix_scale = 1: fixed = %d", fixed);
        P.pb.fix_scale = -1;
        CHECK(!nofov_check(&P.pb, &P.opts, fixed) && fixed == 0, "fix_scale = -1, a motion above both thresholds: fixed = %d", fixed);
        motion(0.049, 1.0, P.Tm);
        CHECK(!nofov_check(&P.pb, &P.opts, fixed) && fixed == 1, "fix_scale = -1, a small rotation: fixed = %d", fixed);
    }
    // the refusals, one problem per text
    { Problem P; P.pb.cam0 = 2; refused("nofov_scale: bad argument", P); }
    { Problem P; int fixed = 0; const char* got = nofov_check(&P.pb, nullptr, fixed); CHECK(got && !strcmp(got, "nofov_scale: bad argument"), "null options accepted"); }
    { Problem P; P.pb.n_lmk = 65537; refused("nofov_scale: more than 65536 landmarks", P); }
    { Problem P; P.optr[2] = 2; refused("nofov_scale: lmk_obs_ptr does not span n_obs", P); }
    { Problem P; P.optr[1] = 4; refused("nofov_scale: lmk_obs_ptr is not monotone", P); }
    {
        Problem P;
        P.pb.n_lmk = 1; P.pb.n_obs = 17; P.optr = {0, 17}; P.ofr.assign(17, 0); P.ocam.assign(17, 0); P.obear.assign(51, 0.5);
        P.pb.lmk_obs_ptr = P.optr.data(); P.pb.obs_frame = P.ofr.data(); P.pb.obs_cam = P.ocam.data(); P.pb.obs_bearing = P.obear.data();
        refused("nofov_scale: more than 16 angular factors on a landmark", P);
    }
    { Problem P; P.scam[1] = 2; refused("nofov_scale: scale_cam out of range", P); }
    { Problem P; P.pb.n_lmk = 0; P.pb.n_obs = 1; refused("nofov_scale: observations without landmarks", P); }
    { Problem P; P.ofr[2] = 2; refused("nofov_scale: observation index out of range", P); }
    { Problem P; P.pb.n_lmk = 0; P.pb.n_obs = 0; P.pb.fix_scale = 1; refused("nofov_scale: no landmark and a constant scale: nothing to solve", P); }
    {   // ... and n_lmk = 0 with a free scale is a problem
        Problem P; P.pb.n_lmk = 0; P.pb.n_obs = 0;
        int fixed = -7;
        CHECK(!nofov_check(&P.pb, &P.opts, fixed) && fixed == 0, "no landmark, free scale: refused");
    }
    printf(fails ? "%d checks failed\n" : "OK\n", fails);
    return fails ? 1 : 0;
}
