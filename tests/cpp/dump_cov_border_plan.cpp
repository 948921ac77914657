// Prints what the host-only planner of the covariance's border route (sadvio_amd/csrc/cov_border_plan.h) makes of a window's
// couplings, for tests/test_cov_border_plan_cpu.py. Host only; a sanitizer build of this program is the place to check the planner.
// Reads from stdin (whitespace separated integers):
//   n_free dpf nb hb_lim fills
//   n_lmk, then per landmark: n, its n observing free key-frames (any order, repeats and -1 for a constant key-frame allowed)
//   n_pair, then per IMU pair or relative-pose factor: a b
// Prints:
//   A answer n_edges hb_core n_core
//   B | the border's free key-frames
//   C | core_of of every free key-frame
//   O | the order [core | border]
#include <cstdio>
#include <cstdlib>

#include "../../sadvio_amd/csrc/cov_border_plan.h"

using namespace sadvio;

static int next_int() {
    int v = 0;
    if (scanf("%d", &v) != 1) { fprintf(stderr, "dump_cov_border_plan: input ends early\n"); exit(2); }
    return v;
}

int main() {
    CovBorderCouplings Cp;
    Cp.n_free = next_int();
    const int dpf = next_int(), nb = next_int(), hb_lim = next_int(), fills = next_int();
    const int n_lmk = next_int();
    std::vector<int> f;
    for (int l = 0; l < n_lmk; l++) {
        const int n = next_int();
        f.resize((size_t)n);
        for (int i = 0; i < n; i++) {
            f[i] = next_int();
            if (f[i] >= Cp.n_free) { fprintf(stderr, "dump_cov_border_plan: key-frame out of range\n"); return 2; }
        }
        Cp.add_landmark(f.data(), n);
    }
    const int n_pair = next_int();
    for (int p = 0; p < n_pair; p++) {
        const int a = next_int(), b = next_int();
        if (a >= Cp.n_free || b >= Cp.n_free) { fprintf(stderr, "dump_cov_border_plan: key-frame out of range\n"); return 2; }
        Cp.add_pair(a, b);
    }
    CovBorderPlan P;
    P.border = {97, 98}; P.core_of = {1}; P.order = {5}; P.hb_core = 77;   // stale contents must not survive
    cov_border_plan(Cp, dpf, nb, hb_lim, fills != 0, P);
    static const char* const names[] = {"OK", "PLAIN", "FILLED", "TOO_WIDE", "CORE_SHAPE"};
    printf("A %s %d %d %d\n", names[P.answer], P.n_edges, P.hb_core, P.n_core());
    printf("B |"); for (int k : P.border) printf(" %d", k); printf("\n");
    printf("C |"); for (int k : P.core_of) printf(" %d", k); printf("\n");
    printf("O |"); for (int k : P.order) printf(" %d", k); printf("\n");
    return 0;
}
