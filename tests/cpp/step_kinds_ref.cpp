// TEST INFRASTRUCTURE — the probe of the one-step check (tests/lm_step_common.py) for every problem kind: the windowed solve() with
// per-landmark constness (limo_ba_solve_fixed_landmarks) and the adjustPoseOnly problem with its speed prior
// (limo_ba_adjust_pose_only).  oracle_ba_step_probe / oracle_ba_problem_cost_at know only build_solve_problem; here the same
// StepProbe is taken from build_pose_only_problem, or from build_solve_problem with the flagged landmarks' blocks set constant.
// The oracle is included as it stands (through the fixed-landmark checker, whose ref_ba_solve_fixed this library exports with its own
// copy of the oracle's iteration tables: the oracle as the second CPU implementation of a fixed-landmark step).  Built by
// tests/lm_step_common.py with the oracle's flags, together with oracle/ceres_like.cpp, into tests/cpp/_build/.
#include "fixed_lm_ref.cpp"

namespace {

// ProblemAt (kba_oracle.cpp) for a problem kind: BUILT at the parameters of `w` on private copies of the parameter arrays, flagged
// landmarks set constant after the build, then the arrays take the values of `at` (null: they stay at w).
struct KindAt {
    std::vector<double> pose, dir, dist, lm;
    limo_ba_window c;
    Built B;
    KindAt(const limo_ba_window& w, const limo_ba_options& o, const double* const* at, bool pose_only, const limo_speed_prior* prior,
           const uint8_t* lm_fixed)
        : pose(w.kf_pose, w.kf_pose + 7 * (size_t)w.n_kf), dir(w.kf_plane_dir, w.kf_plane_dir + 3 * (size_t)w.n_kf),
          dist(w.kf_plane_dist, w.kf_plane_dist + w.n_kf), lm(w.lm_pos, w.lm_pos + 3 * (size_t)w.n_lm), c(w) {
        c.kf_pose = pose.data();
        c.kf_plane_dir = dir.data();
        c.kf_plane_dist = dist.data();
        c.lm_pos = lm.data();
        if (pose_only)
            build_pose_only_problem(c, prior, o, B);
        else
            build_solve_problem(c, o, B);
        if (lm_fixed)
            for (int l = 0; l < c.n_lm; ++l)
                if (lm_fixed[l])
                    if (ParamBlock* p = B.problem.Get(c.lm_pos + 3 * l)) p->constant = true;
        if (at) {
            std::copy(at[0], at[0] + pose.size(), pose.begin());
            std::copy(at[1], at[1] + dir.size(), dir.begin());
            std::copy(at[2], at[2] + dist.size(), dist.begin());
            std::copy(at[3], at[3] + lm.size(), lm.begin());
        }
    }
};

bool kind_valid(const limo_ba_window* w, const limo_ba_options* o, int pose_only) { return w && o && w->n_kf >= 1 && (!pose_only || w->n_kf == 1); }

}  // namespace

extern "C" {

// oracle_ba_step_probe (see there for the outputs) with the problem kind: pose_only != 0 the adjustPoseOnly problem of the window
// (n_kf == 1) with `prior` (null or speed_weight <= 0: none), else the solve() problem; lm_fixed: null, or n_lm flags - != 0: the
// landmark's parameter block is constant.  Returns 1 when the solve takes no step (nothing to optimise, among others).
int kinds_step_probe(const limo_ba_window* w, const limo_ba_options* o, const double* const* at4, int pose_only, const limo_speed_prior* prior,
                     const uint8_t* lm_fixed, int32_t* sizes3, double* J, double* r, double* D, double* y, double* scale, int32_t* colmap,
                     double* costs2) {
    if (!kind_valid(w, o, pose_only) || !sizes3) return LIMO_ERR_INVALID;
    KindAt P(*w, *o, at4, pose_only != 0, prior, lm_fixed);
    SolverOptions so = make_options(*o, 1, 1);
    so.max_num_iterations = 1;
    StepProbe probe;
    so.probe = &probe;
    SolverSummary sum;
    Solve(so, &P.B.problem, &sum);
    if (!probe.filled) return 1;
    if (probe.y.empty()) probe.y.assign(probe.num_eff, std::numeric_limits<double>::quiet_NaN());
    sizes3[0] = probe.num_residuals;
    sizes3[1] = probe.num_eff;
    sizes3[2] = probe.num_e;
    if (J) std::memcpy(J, probe.J.data(), sizeof(double) * probe.J.size());
    if (r) std::memcpy(r, probe.r.data(), sizeof(double) * probe.r.size());
    if (D) std::memcpy(D, probe.D.data(), sizeof(double) * probe.D.size());
    if (y) std::memcpy(y, probe.y.data(), sizeof(double) * probe.y.size());
    if (scale) std::memcpy(scale, probe.scale.data(), sizeof(double) * probe.scale.size());
    if (colmap) {
        const limo_ba_window& c = P.c;
        for (int i = 0; i < probe.num_eff; ++i) {
            const double* u = probe.col_user[i];
            int kind = -1, index = -1;
            if (u >= c.lm_pos && u < c.lm_pos + 3 * (size_t)c.n_lm) {
                kind = 0;
                index = (int)((u - c.lm_pos) / 3);
            } else if (u >= c.kf_pose && u < c.kf_pose + 7 * (size_t)c.n_kf) {
                kind = 1;
                index = (int)((u - c.kf_pose) / 7);
            } else if (u >= c.kf_plane_dir && u < c.kf_plane_dir + 3 * (size_t)c.n_kf) {
                kind = 2;
                index = (int)((u - c.kf_plane_dir) / 3);
            } else if (u >= c.kf_plane_dist && u < c.kf_plane_dist + c.n_kf) {
                kind = 3;
                index = (int)(u - c.kf_plane_dist);
            }
            colmap[3 * i + 0] = kind;
            colmap[3 * i + 1] = index;
            colmap[3 * i + 2] = probe.col_comp[i];
        }
    }
    if (costs2) {
        costs2[0] = probe.cost;
        costs2[1] = probe.fixed_cost;
    }
    return LIMO_OK;
}

// oracle_ba_problem_cost_at for the problem kind: the total cost (with loss, constant blocks included) of the problem built at `w`,
// evaluated at the parameter arrays of at4 (null: at w).
int kinds_problem_cost_at(const limo_ba_window* w, const limo_ba_options* o, const double* const* at4, int pose_only, const limo_speed_prior* prior,
                          const uint8_t* lm_fixed, double* cost) {
    if (!kind_valid(w, o, pose_only) || !cost) return LIMO_ERR_INVALID;
    KindAt P(*w, *o, at4, pose_only != 0, prior, lm_fixed);
    std::vector<ResidualBlock*> all;
    for (auto& b : P.B.problem.blocks) all.push_back(b.get());
    return P.B.problem.Evaluate(all, true, cost, nullptr) ? LIMO_OK : 1;
}

// The depth, reprojection and ground-plane block counts of the problem kind (limo_ba_report::n_depth_blocks ..).
int kinds_block_counts(const limo_ba_window* w, const limo_ba_options* o, int pose_only, const limo_speed_prior* prior, int32_t* counts3) {
    if (!kind_valid(w, o, pose_only) || !counts3) return LIMO_ERR_INVALID;
    KindAt P(*w, *o, nullptr, pose_only != 0, prior, nullptr);
    counts3[0] = P.B.n_depth;
    counts3[1] = P.B.n_repr;
    counts3[2] = P.B.n_gp;
    return LIMO_OK;
}

// the iteration table of the last ref_ba_solve_fixed of THIS library on this thread (oracle_last_iteration_log's entries)
int kinds_last_iteration_log(int32_t cap, limo_ba_iteration* out) { return oracle_last_iteration_log(cap, out); }

}  // extern "C"
