// kba_window_options.hpp — the host rule of limo_ba_batch_solve_each / limo_ba_adjust_pose_only_batch_each (limo_hip.h): which
// fields of limo_ba_options may differ between the windows of one batch, how a refusal reads, when an array is "uniform" (no table
// at all), and the record a window's own options turn into (kba_layout.hpp:WinOpts).  No HIP in here: the library includes it,
// and tests/cpp/test_window_options.cpp compiles it with a host compiler.
#pragma once
#include <cmath>
#include <cstring>
#include <string>
#include <vector>

#include "kba_pack.hpp"

namespace kba {

// The fields that may differ from window to window: the numeric members of the reference's OutlierRejectionOptions
// (bundle_adjuster_keyframes.hpp:79-89).  Every kernel that reads them knows its window.
// Everything else - the schedule (num_trim_rounds, trim_solver_iterations, max_num_iterations, max_solver_time_sec),
// min_landmarks_for_trimming / minimum_number_residual_groups and the LM constants - decides launches or is read by kernels that
// serve many windows with one set of constants: bitwise equal in all entries.
template <typename T>
inline bool same_bits(const T& a, const T& b) {
    return std::memcmp(&a, &b, sizeof(T)) == 0;
}

// The first field of `o` that must equal `ref`'s and does not (its name), or null.
inline const char* window_options_fixed_diff(const limo_ba_options& ref, const limo_ba_options& o) {
#define KBA_WOPT_FIXED(f) \
    if (!same_bits(ref.f, o.f)) return #f;
    KBA_WOPT_FIXED(num_trim_rounds)
    KBA_WOPT_FIXED(trim_solver_iterations)
    KBA_WOPT_FIXED(min_landmarks_for_trimming)
    KBA_WOPT_FIXED(minimum_number_residual_groups)
    KBA_WOPT_FIXED(max_num_iterations)
    KBA_WOPT_FIXED(max_solver_time_sec)
    KBA_WOPT_FIXED(function_tolerance)
    KBA_WOPT_FIXED(gradient_tolerance)
    KBA_WOPT_FIXED(parameter_tolerance)
    KBA_WOPT_FIXED(initial_trust_region_radius)
    KBA_WOPT_FIXED(max_trust_region_radius)
    KBA_WOPT_FIXED(min_trust_region_radius)
    KBA_WOPT_FIXED(min_lm_diagonal)
    KBA_WOPT_FIXED(max_lm_diagonal)
    KBA_WOPT_FIXED(min_relative_decrease)
    KBA_WOPT_FIXED(max_num_consecutive_invalid_steps)
    KBA_WOPT_FIXED(jacobi_scaling)
#undef KBA_WOPT_FIXED
    return nullptr;
}

// The four fields that may differ are all bitwise equal.
inline bool window_options_free_equal(const limo_ba_options& a, const limo_ba_options& b) {
    return same_bits(a.depth_thres, b.depth_thres) && same_bits(a.reprojection_thres, b.reprojection_thres) &&
           same_bits(a.depth_quantile, b.depth_quantile) && same_bits(a.reprojection_quantile, b.reprojection_quantile);
}
inline bool window_options_equal(const limo_ba_options& a, const limo_ba_options& b) {
    return window_options_free_equal(a, b) && !window_options_fixed_diff(a, b);
}

// A per-window value no solve can use: a threshold or quantile that is not a finite number (its name), or null.
inline const char* window_options_not_finite(const limo_ba_options& o) {
    if (!std::isfinite(o.depth_thres)) return "depth_thres";
    if (!std::isfinite(o.reprojection_thres)) return "reprojection_thres";
    if (!std::isfinite(o.depth_quantile)) return "depth_quantile";
    if (!std::isfinite(o.reprojection_quantile)) return "reprojection_quantile";
    return nullptr;
}

// The rule over an array: LIMO_OK, or LIMO_ERR_INVALID with `err` naming the first offending window and field ("window 3:
// max_num_iterations").  *uniform: every entry equals entry 0 - the call is the one-options call, no table exists.
inline int check_window_options(int n_win, int n_opts, const limo_ba_options* opts, bool* uniform, std::string& err) {
    *uniform = true;
    if (!opts) {
        err = "opts is NULL";
        return LIMO_ERR_INVALID;
    }
    if (n_opts != n_win) {
        err = "n_opts (" + std::to_string(n_opts) + ") differs from the number of windows (" + std::to_string(n_win) + ")";
        return LIMO_ERR_INVALID;
    }
    for (int w = 0; w < n_opts; ++w) {
        if (const char* f = window_options_not_finite(opts[w])) {
            err = "window " + std::to_string(w) + ": " + f + " is not finite";
            return LIMO_ERR_INVALID;
        }
        if (const char* f = window_options_fixed_diff(opts[0], opts[w])) {
            err = "window " + std::to_string(w) + ": " + f;
            return LIMO_ERR_INVALID;
        }
        if (!window_options_free_equal(opts[0], opts[w])) *uniform = false;
    }
    return LIMO_OK;
}

// The record of one window: the six members as make_consts of ITS options computes them.
inline WinOpts window_options_record(const limo_ba_options& o) {
    const SolveConsts c = make_consts(o);
    WinOpts r;
    std::memset(&r, 0, sizeof(r));
    r.a_rep = c.a_rep;
    r.a_dep = c.a_dep;
    r.inv_a_rep2 = c.inv_a_rep2;
    r.inv_a_dep2 = c.inv_a_dep2;
    r.depth_quantile = c.depth_quantile;
    r.reprojection_quantile = c.reprojection_quantile;
    return r;
}
// The table of an array that passed check_window_options: empty when it is uniform.
inline void window_options_table(int n, const limo_ba_options* opts, bool uniform, std::vector<WinOpts>& out) {
    out.clear();
    if (uniform) return;
    out.reserve(n);
    for (int w = 0; w < n; ++w) out.push_back(window_options_record(opts[w]));
}

}  // namespace kba
