// solve_opts.h — the caller's solve options as the kernels take them, and the summary tail the one-launch solvers write. Plain
// C++17 without the HIP runtime or the handle (tests/cpp/test_solve_opts.cpp).
#pragma once
#include "../../include/sadvio_ba.h"
#include "ba_types.h"

// The twelve fields every solver shares. Nothing else of `o` is written: huber_a, max_time_ticks and the padding are the caller's
// (sadvio_ba_solve zeroes the struct first, its bytes are part of the graph key; vi_init and nofov_scale leave huber_a at zero).
inline void solve_opts_from(const sadvio_solve_options& opts, sadvio::SolveOpts& o) {
    o.max_num_iterations = opts.max_num_iterations; o.jacobi_scaling = opts.jacobi_scaling;
    o.max_num_consecutive_invalid_steps = opts.max_num_consecutive_invalid_steps;
    o.function_tolerance = opts.function_tolerance; o.gradient_tolerance = opts.gradient_tolerance;
    o.parameter_tolerance = opts.parameter_tolerance; o.initial_radius = opts.initial_trust_region_radius;
    o.max_radius = opts.max_trust_region_radius; o.min_radius = opts.min_trust_region_radius;
    o.min_lm_diagonal = opts.min_lm_diagonal; o.max_lm_diagonal = opts.max_lm_diagonal;
    o.min_relative_decrease = opts.min_relative_decrease;
}

// initial_cost final_cost radius iterations termination n_success n_unsuccess, as k_viinit and k_nofov leave them behind their results
inline void summary_from_tail(const double* s7, sadvio_solve_summary& S) {
    S.initial_cost = s7[0]; S.final_cost = s7[1]; S.final_radius = s7[2]; S.iterations = (int)s7[3]; S.termination = (int)s7[4];
    S.num_successful_steps = (int)s7[5]; S.num_unsuccessful_steps = (int)s7[6];
}
