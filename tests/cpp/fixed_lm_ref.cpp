// TEST INFRASTRUCTURE — the checker of the fixed-landmark solve (limo_ba_solve_fixed_landmarks): the oracle's own problem build
// and solveTrimmed loop (oracle/kba_oracle.cpp, included as it stands) with the flagged landmarks' parameter blocks set constant
// - what BundleAdjusterKeyframes::deactivateLandmarks does to a problem (bundle_adjuster_keyframes.cpp:262-269).  Built by
// tests/fixed_lm_common.py with the oracle's flags, together with oracle/ceres_like.cpp, into tests/cpp/_build/.
#include "../../oracle/kba_oracle.cpp"

static int g_ref_threads = 1;

extern "C" {

// threads of the checker's residual evaluation and Schur elimination (oracle_ba_solve's num_threads arguments)
void ref_set_threads(int n) { g_ref_threads = n < 1 ? 1 : n; }

// oracle_ba_solve with per-landmark constness.  fixed: NULL or n_lm flags in the caller's landmark order.
int ref_ba_solve_fixed(limo_ba_window* w, const uint8_t* fixed, const limo_ba_options* o, limo_ba_report* rep) {
    if (!w || !o) return LIMO_ERR_INVALID;
    if (w->n_kf < 1) return LIMO_ERR_NOT_ENOUGH_KF;
    Built B;
    build_solve_problem(*w, *o, B);
    if (fixed)
        for (int l = 0; l < w->n_lm; ++l)
            if (fixed[l])
                if (ParamBlock* p = B.problem.Get(w->lm_pos + 3 * l)) p->constant = true;
    std::vector<int> number_iterations;  // (as oracle_ba_solve makes them)
    if (w->n_lm > o->min_landmarks_for_trimming)
        for (int i = 0; i < o->num_trim_rounds; ++i) number_iterations.push_back(o->trim_solver_iterations);
    std::vector<std::pair<IdMap*, double>> input;
    input.push_back({&B.depth, o->depth_quantile});
    input.push_back({&B.repr, o->reprojection_quantile});
    input.push_back({&B.gp, 1.0});
    TrimResult R = solve_trimmed(number_iterations, input, B.problem, make_options(*o, g_ref_threads, g_ref_threads), (size_t)o->minimum_number_residual_groups);
    fill_report(R, B, rep, nullptr);
    return LIMO_OK;
}

// landmark indices trimmed by the last ref_ba_solve_fixed on this thread (this library's own copy of the oracle's list)
int ref_last_trimmed(int32_t* out, int cap) { return oracle_last_trimmed(out, cap); }

}  // extern "C"
