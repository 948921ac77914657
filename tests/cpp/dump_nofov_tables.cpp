// Prints the constant tables sadvio_amd/csrc/nofov_plan.h makes of a problem, so that tests/test_capi_host_cpu.py can compare them
// with the twin's (tests/nofov_helpers.py). Host only.
// Reads from stdin: n_frames n_cam cam0, then frame_T_f_w [n_frames][12], cam_T_s_f [n_cam][12], T_cam0_cam0p [12] (%la each).
// Prints one line per frame ("F" and its 39 numbers) and one per camera ("C" and its 15), %.17g each.
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "../../sadvio_amd/csrc/nofov_plan.h"

static void read(std::vector<double>& v) {
    for (double& x : v)
        if (scanf("%la", &x) != 1) { fprintf(stderr, "dump_nofov_tables: input ends early\n"); exit(2); }
}

int main() {
    sadvio_nofov_problem pb = {};
    if (scanf("%d %d %d", &pb.n_frames, &pb.n_cam, &pb.cam0) != 3 || pb.n_frames < 1 || pb.n_cam < 1 || pb.cam0 < 0 || pb.cam0 >= pb.n_cam) return 2;
    std::vector<double> frames(12 * (size_t)pb.n_frames), cams(12 * (size_t)pb.n_cam), Tm(12);
    read(frames); read(cams); read(Tm);
    pb.frame_T_f_w = frames.data(); pb.cam_T_s_f = cams.data(); pb.T_cam0_cam0p = Tm.data();
    std::vector<double> ftab(NOFOV_PLAN_FTAB * (size_t)pb.n_frames), ctab(NOFOV_PLAN_CTAB * (size_t)pb.n_cam);
    nofov_tables(&pb, ftab.data(), ctab.data());
    for (int k = 0; k < pb.n_frames; k++) {
        printf("F");
        for (int i = 0; i < NOFOV_PLAN_FTAB; i++) printf(" %.17g", ftab[NOFOV_PLAN_FTAB * (size_t)k + i]);
        printf("\n");
    }
    for (int c = 0; c < pb.n_cam; c++) {
        printf("C");
        for (int i = 0; i < NOFOV_PLAN_CTAB; i++) printf(" %.17g", ctab[NOFOV_PLAN_CTAB * (size_t)c + i]);
        printf("\n");
    }
    return 0;
}
