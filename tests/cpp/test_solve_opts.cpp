// Stand-alone check of sadvio_amd/csrc/solve_opts.h (host only; built and run by tests/test_capi_host_cpu.py): the twelve shared
// option fields arrive in SolveOpts under the right names and nothing else of it is written; the seven-number tail of the one-launch
// solvers lands in the right summary fields and nothing else of the summary is written.
#include <cstddef>
#include <cstdio>
#include <cstring>

#include "../../sadvio_amd/csrc/solve_opts.h"

static int fails = 0;
#define CHECK(cond, ...) do { if (!(cond)) { fails++; printf("MISMATCH %s:%d: ", __FILE__, __LINE__); printf(__VA_ARGS__); printf("\n"); } } while (0)

int main() {
    sadvio_solve_options in;
    in.max_num_iterations = 101; in.jacobi_scaling = 102; in.max_num_consecutive_invalid_steps = 103; in.reserved = 104;
    in.function_tolerance = 1.05; in.gradient_tolerance = 1.06; in.parameter_tolerance = 1.07; in.initial_trust_region_radius = 1.08;
    in.max_trust_region_radius = 1.09; in.min_trust_region_radius = 1.10; in.min_lm_diagonal = 1.11; in.max_lm_diagonal = 1.12;
    in.min_relative_decrease = 1.13; in.huber_a = 1.14; in.max_solver_time_in_seconds = 1.15;
    sadvio::SolveOpts o, before;
    memset(&before, 0xab, sizeof(before));
    o = before;
    solve_opts_from(in, o);
    CHECK(o.max_num_iterations == 101 && o.jacobi_scaling == 102 && o.max_num_consecutive_invalid_steps == 103, "the integer fields");
    CHECK(o.function_tolerance == 1.05 && o.gradient_tolerance == 1.06 && o.parameter_tolerance == 1.07, "the tolerances");
    CHECK(o.initial_radius == 1.08 && o.max_radius == 1.09 && o.min_radius == 1.10, "the radii");
    CHECK(o.min_lm_diagonal == 1.11 && o.max_lm_diagonal == 1.12 && o.min_relative_decrease == 1.13, "the diagonal bounds and the decrease");
    CHECK(!memcmp(&o.pad, &before.pad, sizeof(o.pad)) && !memcmp(&o.huber_a, &before.huber_a, sizeof(double)) && !memcmp(&o.max_time_ticks, &before.max_time_ticks, sizeof(double)),
          "pad, huber_a or max_time_ticks was written");
    // the twelve fields and those three are the whole struct
    static_assert(sizeof(sadvio::SolveOpts) == 4 * sizeof(int) + 11 * sizeof(double), "SolveOpts has a field this test does not know");

    const double tail[7] = {1.5, 2.5, 3.5, 4.0, 5.0, 6.0, 7.0};
    sadvio_solve_summary S;
    memset(&S, 0, sizeof(S));
    S.fixed_cost = 9.5;
    summary_from_tail(tail, S);
    CHECK(S.initial_cost == 1.5 && S.final_cost == 2.5 && S.final_radius == 3.5 && S.iterations == 4 && S.termination == 5 && S.num_successful_steps == 6 &&
          S.num_unsuccessful_steps == 7, "the summary fields");
    CHECK(S.fixed_cost == 9.5, "fixed_cost was written");
    static_assert(sizeof(sadvio_solve_summary) == 4 * sizeof(int32_t) + 4 * sizeof(double), "sadvio_solve_summary has a field this test does not know");
    printf(fails ? "%d checks failed\n" : "OK\n", fails);
    return fails ? 1 : 0;
}
