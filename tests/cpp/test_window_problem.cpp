// Host-only checks of the problem's rules (kba_pack.hpp:build_window_problem): which residual and parameter blocks a window has,
// each case against values written out from the rule it restates (bundle_adjuster_keyframes.cpp: ground-plane wiring :517-562,
// scale / ground-plane regularisers and constness :704-736, :890-904).  Stand-alone program, built with
// -fsanitize=address,undefined by tests/test_window_problem_cpu.py together with kba_pack.cpp.  Nothing here packs a batch, except
// the last case (an option pair pack_windows refuses).
#include <cmath>
#include <cstdio>
#include <cstring>
#include <string>
#include <vector>

#include "../../limo_amd/csrc/kba_pack.hpp"

using namespace kba;

static int g_failed = 0, g_checks = 0;
#define CHECK(cond)                                                        \
    do {                                                                   \
        ++g_checks;                                                        \
        if (!(cond)) {                                                     \
            ++g_failed;                                                    \
            std::printf("FAILED %s:%d: %s\n", __FILE__, __LINE__, #cond);  \
        }                                                                  \
    } while (0)

// A window built by hand.  Keyframes have the identity rotation unless a case sets one, so that the distance of landmark p to
// keyframe k (|R_k p + t_k|) is |p + t_k| and can be written down.
struct Win {
    std::vector<double> pose, pdir, pdist, cam, lm, weight;
    std::vector<int32_t> fix, okf, olm, ocam;
    std::vector<uint8_t> ground;
    std::vector<float> u, v, d;
    limo_ba_window w;

    Win(int n_kf, int n_lm, int n_cam) {
        pose.assign((size_t)7 * n_kf, 0.0);
        for (int k = 0; k < n_kf; ++k) pose[7 * k] = 1.0;
        pdir.assign((size_t)3 * n_kf, 0.0);
        for (int k = 0; k < n_kf; ++k) pdir[3 * k + 1] = 1.0;
        pdist.assign(n_kf, 1.7);
        fix.assign(n_kf, LIMO_FIX_NONE);
        for (int c = 0; c < n_cam; ++c) {
            const double q[10] = {700.0, 600.0, 180.0, 1.0, 0.0, 0.0, 0.0, 0.5 * c, 0.0, 0.0};
            cam.insert(cam.end(), q, q + 10);
        }
        lm.assign((size_t)3 * n_lm, 0.0);
        for (int l = 0; l < n_lm; ++l) lm[3 * l + 2] = 100.0 + l;  // (far from every keyframe: no ground-plane row by accident)
        weight.assign(n_lm, 1.0);
        ground.assign(n_lm, 0);
    }
    void set_t(int k, double x, double y, double z) {
        pose[7 * k + 4] = x;
        pose[7 * k + 5] = y;
        pose[7 * k + 6] = z;
    }
    void set_lm(int l, double x, double y, double z, bool is_ground) {
        lm[3 * l] = x;
        lm[3 * l + 1] = y;
        lm[3 * l + 2] = z;
        ground[l] = is_ground ? 1 : 0;
    }
    void obs(int k, int l, int c, float depth) {
        okf.push_back(k);
        olm.push_back(l);
        ocam.push_back(c);
        u.push_back(600.0f + l);
        v.push_back(180.0f + k);
        d.push_back(depth);
    }
    const limo_ba_window& get() {
        std::memset(&w, 0, sizeof(w));
        w.n_kf = (int32_t)pdist.size();
        w.n_cam = (int32_t)(cam.size() / 10);
        w.n_lm = (int32_t)weight.size();
        w.n_obs = (int32_t)olm.size();
        w.kf_pose = pose.data();
        w.kf_plane_dir = pdir.data();
        w.kf_plane_dist = pdist.data();
        w.kf_fixation = fix.data();
        w.cam = cam.data();
        w.lm_pos = lm.data();
        w.lm_weight = weight.data();
        w.lm_is_ground = ground.data();
        w.obs_kf = okf.data();
        w.obs_lm = olm.data();
        w.obs_cam = ocam.data();
        w.obs_u = u.data();
        w.obs_v = v.data();
        w.obs_d = d.data();
        return w;
    }
};

static limo_ba_options g_opts;

static WindowProblem solve_problem(Win& W) { return build_window_problem(W.get(), g_opts, PackOptions(), 0); }

using SlotMask = decltype(WindowProblem::present);
static bool pose_block(const SlotMask& m, int k, int want) {
    for (int i = 0; i < 6; ++i)
        if (m[k * kCamSlots + i] != want) return false;
    return true;
}
static bool plane_dir_block(const SlotMask& m, int k, int want) {
    for (int i = 6; i < 9; ++i)
        if (m[k * kCamSlots + i] != want) return false;
    return true;
}

// A weight of the ground-plane rule is 10 (1 - d / 25) with d the distance written into the case: a handful of roundings of
// numbers of size <= 25, far below 1e-12.
static bool near(double a, double b) { return std::fabs(a - b) <= 1e-12; }

static void ground_plane() {
    {   // 24.9 m from the nearest keyframe: a row with weight 10 (1 - 24.9 / 25); 25 m: none
        Win W(2, 3, 1);
        W.set_t(1, 0.0, 0.0, 10.0);               // keyframe 1 is 10 m further from everything on the +z axis
        W.set_lm(0, 0.0, 0.0, 24.9, true);        // |p + t_0| = 24.9, |p + t_1| = 34.9
        W.set_lm(1, 0.0, 0.0, 25.0, true);        // 25 and 35
        W.set_lm(2, 0.0, 0.0, 3.0, false);        // near, but not a ground landmark
        const WindowProblem pr = solve_problem(W);
        CHECK(pr.rc == LIMO_OK);
        CHECK(pr.gp.size() == 1);
        if (pr.gp.size() == 1) {
            CHECK(pr.gp[0].kf == 0 && pr.gp[0].lm == 0);
            CHECK(near(pr.gp[0].w, 10. * (1. - 24.9 / 25.)));
        }
    }
    {   // a keyframe with kf_plane_dist < -10 is never chosen, however near; -10 itself still is
        Win W(3, 2, 1);
        W.set_t(0, 0.0, 0.0, 0.0);
        W.set_t(1, 0.0, 0.0, 15.0);
        W.set_t(2, 0.0, 0.0, 17.0);
        W.set_lm(0, 0.0, 0.0, 5.0, true);  // 5 m, 20 m, 22 m
        W.set_lm(1, 0.0, 3.0, 4.0, true);  // 5 m from keyframe 0 again (3-4-5)
        W.pdist[0] = -10.5;
        WindowProblem pr = solve_problem(W);
        CHECK(pr.gp.size() == 2);
        if (pr.gp.size() == 2) {
            CHECK(pr.gp[0].kf == 1 && pr.gp[0].lm == 0 && near(pr.gp[0].w, 10. * (1. - 20. / 25.)));
            CHECK(pr.gp[1].kf == 1 && pr.gp[1].lm == 1);  // rows in landmark order
        }
        W.pdist[0] = -10.0;
        pr = solve_problem(W);
        CHECK(pr.gp.size() == 2);
        if (pr.gp.size() == 2) CHECK(pr.gp[0].kf == 0 && near(pr.gp[0].w, 10. * (1. - 5. / 25.)) && pr.gp[1].kf == 0 && near(pr.gp[1].w, 8.0));
        // all keyframes below -10: no row, and no ground-plane regulariser
        W.pdist.assign(3, -10.001);
        pr = solve_problem(W);
        CHECK(pr.rc == LIMO_OK && pr.gp.empty() && !pr.has_gp_reg);
    }
}

// n_dep landmarks (one at least) observed with a depth in keyframe 0, n_gp ground landmarks (5 m from keyframe 0, further from
// the others) behind them; with a second keyframe, up to two observations without a depth (0 and negative: neither counts)
static Win scale_window(int n_kf, int n_dep, int n_gp) {
    const int n_seen = std::max(1, n_dep);
    Win W(n_kf, n_seen + n_gp, 1);
    for (int k = 1; k < n_kf; ++k) W.set_t(k, 0.0, 0.0, 2.0 * k);
    for (int l = 0; l < n_dep; ++l) W.obs(0, l, 0, 7.5f);
    if (n_kf > 1) {
        W.obs(1, 0, 0, 0.0f);
        if (n_seen > 1) W.obs(1, n_seen - 1, 0, -1.0f);
    }
    for (int g = 0; g < n_gp; ++g) W.set_lm(n_seen + g, 0.0, 0.0, 5.0, true);
    return W;
}

static void scale_regulariser() {
    {   // n_depth <= 10 and n_gp <= 10: weight 1000 (ten of each: landmarks 2 .. 9 are observed AND ground landmarks)
        Win W(2, 12, 1);
        W.set_t(1, 0.0, 0.0, 2.0);
        for (int l = 0; l < 10; ++l) W.obs(l % 2, l, 0, 6.0f);
        for (int g = 0; g < 10; ++g) W.set_lm(2 + g, 0.0, 0.0, 5.0, true);
        const WindowProblem pr = solve_problem(W);
        CHECK(pr.n_depth == 10 && pr.gp.size() == 10 && pr.n_repr == 10);
        CHECK(pr.has_scale_reg && pr.scale_w == 1000.);
    }
    {   // n_depth = 11, n_gp = 0: 1000 / 11
        Win W = scale_window(2, 11, 0);
        const WindowProblem pr = solve_problem(W);
        CHECK(pr.n_depth == 11 && pr.gp.empty() && pr.n_repr == 13);
        CHECK(pr.has_scale_reg && pr.scale_w == 1000. / 11.);
    }
    {   // n_gp = 11, n_depth = 1: 1000 / 12
        Win W = scale_window(3, 1, 11);
        const WindowProblem pr = solve_problem(W);
        CHECK(pr.n_depth == 1 && pr.gp.size() == 11);
        CHECK(pr.has_scale_reg && pr.scale_w == 1000. / 12.);
    }
    {   // more than 10 of either with n_gp >= 30: none; 29: still one
        Win W = scale_window(2, 0, 30);
        WindowProblem pr = solve_problem(W);
        CHECK(pr.n_depth == 0 && pr.gp.size() == 30);
        CHECK(!pr.has_scale_reg && pr.scale_w == 0.0);
        W = scale_window(2, 11, 30);
        pr = solve_problem(W);
        CHECK(pr.n_depth == 11 && pr.gp.size() == 30 && !pr.has_scale_reg);
        W = scale_window(2, 0, 29);
        pr = solve_problem(W);
        CHECK(pr.gp.size() == 29 && pr.has_scale_reg && pr.scale_w == 1000. / 29.);
    }
    {   // n_kf = 1: none (and no ground-plane regulariser either)
        Win W = scale_window(1, 2, 3);
        const WindowProblem pr = solve_problem(W);
        CHECK(pr.rc == LIMO_OK && pr.gp.size() == 3 && !pr.has_scale_reg && !pr.has_gp_reg);
    }
    {   // s0 = norm of the relative translation of the first two poses = the distance of their camera centres c = -R^T t;
        // rotations about y by a: R = [c 0 s; 0 1 0; -s 0 c], quaternion (cos a/2, 0, sin a/2, 0)
        Win W = scale_window(3, 2, 0);
        const double a[2] = {0.2, -0.1}, t[2][3] = {{1.0, 0.5, -2.0}, {-0.5, 0.25, 3.0}};
        double c[2][3];
        for (int k = 0; k < 2; ++k) {
            W.pose[7 * k] = std::cos(a[k] / 2);
            W.pose[7 * k + 2] = std::sin(a[k] / 2);
            W.set_t(k, t[k][0], t[k][1], t[k][2]);
            const double co = std::cos(a[k]), si = std::sin(a[k]);
            c[k][0] = -(co * t[k][0] - si * t[k][2]);  // R^T = [c 0 -s; 0 1 0; s 0 c]
            c[k][1] = -t[k][1];
            c[k][2] = -(si * t[k][0] + co * t[k][2]);
        }
        const double s0 = std::sqrt((c[1][0] - c[0][0]) * (c[1][0] - c[0][0]) + (c[1][1] - c[0][1]) * (c[1][1] - c[0][1]) +
                                    (c[1][2] - c[0][2]) * (c[1][2] - c[0][2]));
        const WindowProblem pr = solve_problem(W);
        CHECK(pr.has_scale_reg && near(pr.scale_s0, s0) && s0 > 1.0);
    }
}

static void slots() {
    {   // a LIMO_FIX_POSE keyframe is present but has no free slot; plane slot 9 is free only with n_depth >= 10
        for (int n_dep = 9; n_dep <= 10; ++n_dep) {
            Win W(3, 12, 1);
            for (int k = 0; k < 3; ++k) W.set_t(k, 0.0, 0.0, 1.0 * k);
            for (int l = 0; l < n_dep; ++l) W.obs(l % 3, l, 0, 5.0f);
            for (int l = n_dep; l < 12; ++l) W.obs(l % 3, l, 0, -1.0f);
            W.set_lm(11, 0.0, 0.0, 4.0, true);  // one ground-plane row: every keyframe's plane is in (the ground-plane regulariser)
            W.fix[1] = LIMO_FIX_POSE;
            const WindowProblem pr = solve_problem(W);
            CHECK(pr.n_depth == n_dep && pr.gp.size() == 1 && pr.has_gp_reg);
            for (int k = 0; k < 3; ++k) {
                CHECK(pose_block(pr.present, k, 1) && plane_dir_block(pr.present, k, 1) && pr.present[k * kCamSlots + 9] == 1);
                const int fr = k == 1 ? 0 : 1;
                CHECK(pose_block(pr.free, k, fr) && plane_dir_block(pr.free, k, fr));
                CHECK(pr.free[k * kCamSlots + 9] == (fr && n_dep >= 10 ? 1 : 0));
            }
        }
    }
    {   // a keyframe without observations is held in by the ground-plane regulariser - and is out without one
        for (int with_ground = 0; with_ground < 2; ++with_ground) {
            Win W(3, 4, 1);
            for (int k = 0; k < 3; ++k) W.set_t(k, 0.0, 0.0, 1.0 * k);
            for (int l = 0; l < 3; ++l) W.obs(l % 2, l, 0, -1.0f);  // keyframes 0 and 1 only
            if (with_ground) W.set_lm(3, 0.0, 0.0, 4.0, true);     // (its row hangs on keyframe 0)
            const WindowProblem pr = solve_problem(W);
            CHECK((int)pr.gp.size() == with_ground && pr.has_gp_reg == (with_ground == 1));
            CHECK(pose_block(pr.present, 2, with_ground) && pose_block(pr.free, 2, with_ground));
            CHECK(plane_dir_block(pr.present, 2, with_ground) && pr.present[2 * kCamSlots + 9] == with_ground);
            CHECK(pose_block(pr.present, 0, 1) && pose_block(pr.present, 1, 1));
        }
    }
    {   // the first two poses are held in by the scale regulariser: no observation on them, no ground landmark
        Win W(3, 2, 1);
        W.set_t(1, 0.0, 0.0, 1.0);
        W.obs(2, 0, 0, -1.0f);
        const WindowProblem pr = solve_problem(W);
        CHECK(pr.has_scale_reg && !pr.has_gp_reg);
        for (int k = 0; k < 3; ++k) CHECK(pose_block(pr.present, k, 1) && pose_block(pr.free, k, 1) && plane_dir_block(pr.present, k, 0));
        // ... and with one keyframe more, the fourth one (no observation, not one of the first two) is out
        Win V(4, 2, 1);
        V.obs(2, 0, 0, -1.0f);
        const WindowProblem pv = solve_problem(V);
        CHECK(pose_block(pv.present, 0, 1) && pose_block(pv.present, 1, 1) && pose_block(pv.present, 2, 1) && pose_block(pv.present, 3, 0));
    }
}

static void landmark_states() {
    Win W(2, 6, 1);
    W.set_t(1, 0.0, 0.0, 1.0);
    W.obs(0, 0, 0, -1.0f);             // 0: observed
    /* 1: nothing */                   // 1: unobserved
    W.set_lm(2, 0.0, 0.0, 4.0, true);  // 2: unobserved, with a ground-plane row
    W.obs(1, 3, 0, 2.0f);              // 3: observed and flagged
    /* 4: flagged, unobserved */
    W.set_lm(5, 0.0, 0.0, 6.0, true);  // 5: flagged, ground-plane row only
    const uint8_t want_plain[6] = {1, 0, 1, 1, 0, 1};
    WindowProblem pr = solve_problem(W);
    for (int l = 0; l < 6; ++l) CHECK(pr.lm_state[l] == want_plain[l] && pr.lm_const[l] == 0);
    CHECK(pr.n_const == 0);
    const uint8_t flags[6] = {0, 0, 0, 1, 7, 1};
    const uint8_t* per_window[2] = {nullptr, flags};
    PackOptions po;
    po.lm_fixed = per_window;
    pr = build_window_problem(W.get(), g_opts, po, 1);
    const uint8_t want_fixed[6] = {1, 0, 1, 2, 0, 2};
    for (int l = 0; l < 6; ++l) CHECK(pr.lm_state[l] == want_fixed[l] && pr.lm_const[l] == (flags[l] ? 1 : 0));
    CHECK(pr.n_const == 3 && pr.gp.size() == 2);
    pr = build_window_problem(W.get(), g_opts, po, 0);  // (window 0 has no flag array)
    for (int l = 0; l < 6; ++l) CHECK(pr.lm_state[l] == want_plain[l]);
    // pose-only: every observed landmark is a constant block, no ground-plane rows, flags ignored
    Win V(1, 4, 1);
    V.obs(0, 0, 0, 3.0f);
    V.obs(0, 2, 0, -1.0f);
    V.set_lm(3, 0.0, 0.0, 4.0, true);
    PackOptions pp;
    pp.pose_only = true;
    pp.lm_fixed = per_window;
    pr = build_window_problem(V.get(), g_opts, pp, 1);
    const uint8_t want_pose[4] = {2, 0, 2, 0};
    for (int l = 0; l < 4; ++l) CHECK(pr.lm_state[l] == want_pose[l]);
    CHECK(pr.gp.empty() && pr.n_const == 0 && !pr.has_scale_reg && !pr.has_gp_reg && pr.n_depth == 1 && pr.n_repr == 2);
    CHECK(pose_block(pr.present, 0, 1) && pose_block(pr.free, 0, 1) && plane_dir_block(pr.present, 0, 0));
}

static void views() {
    // three keyframes, two cameras; (keyframe 1, camera 0) carries no observation; the observations come in no order
    Win W(3, 3, 2);
    const int pairs[5][2] = {{2, 1}, {0, 1}, {1, 1}, {2, 0}, {0, 0}};
    for (int i = 0; i < 5; ++i) W.obs(pairs[i][0], i % 3, pairs[i][1], -1.0f);
    W.obs(2, 2, 1, -1.0f);
    W.fix[1] = LIMO_FIX_POSE;
    const int plain[5][2] = {{0, 0}, {0, 1}, {1, 1}, {2, 0}, {2, 1}};  // keyframe, then camera
    auto same = [](const WindowProblem& pr, const int (*want)[2]) {
        if (pr.views.size() != 5) return false;
        for (int v = 0; v < 5; ++v)
            if (pr.views[v].kf != want[v][0] || pr.views[v].cam != want[v][1]) return false;
        return true;
    };
    auto obs_views_fit = [](Win& W, const WindowProblem& pr) {
        if (pr.obs_view.size() != W.okf.size()) return false;
        for (size_t i = 0; i < W.okf.size(); ++i) {
            const int v = pr.obs_view[i];
            if (v < 0 || v >= (int)pr.views.size() || pr.views[v].kf != W.okf[i] || pr.views[v].cam != W.ocam[i]) return false;
        }
        return true;
    };
    const WindowProblem p0 = solve_problem(W);
    CHECK(same(p0, plain) && obs_views_fit(W, p0));
    // a flag set: the views of every LIMO_FIX_POSE keyframe first (here keyframe 1, then also keyframe 2)
    const uint8_t none[3] = {0, 0, 0}, one[3] = {0, 1, 0};
    const uint8_t* arr[1] = {one};
    PackOptions po;
    po.lm_fixed = arr;
    const int first1[5][2] = {{1, 1}, {0, 0}, {0, 1}, {2, 0}, {2, 1}};
    WindowProblem p1 = build_window_problem(W.get(), g_opts, po, 0);
    CHECK(same(p1, first1) && obs_views_fit(W, p1));
    W.fix[2] = LIMO_FIX_POSE;
    const int first12[5][2] = {{1, 1}, {2, 0}, {2, 1}, {0, 0}, {0, 1}};
    p1 = build_window_problem(W.get(), g_opts, po, 0);
    CHECK(same(p1, first12) && obs_views_fit(W, p1));
    // no flag set: exactly the order without the array
    arr[0] = none;
    p1 = build_window_problem(W.get(), g_opts, po, 0);
    CHECK(same(p1, plain) && obs_views_fit(W, p1) && p1.n_const == 0);
    CHECK(p1.obs_view == solve_problem(W).obs_view);
}

static void trimming_prior_and_refusals() {
    {   // do_trim: n_lm > min_landmarks_for_trimming
        limo_ba_options o = g_opts;
        Win W(2, 12, 1);
        o.min_landmarks_for_trimming = 12;
        CHECK(!build_window_problem(W.get(), o, PackOptions(), 0).do_trim);
        o.min_landmarks_for_trimming = 11;
        CHECK(build_window_problem(W.get(), o, PackOptions(), 0).do_trim);
    }
    {   // the pose-only prior is the window's own; speed_weight <= 0: none
        Win W(1, 3, 1);
        W.obs(0, 1, 0, 2.0f);
        limo_speed_prior pri[3];
        std::memset(pri, 0, sizeof(pri));
        const double weight[3] = {0.7, 0.0, -2.0};
        for (int i = 0; i < 3; ++i) {
            pri[i].speed_weight = weight[i];
            pri[i].dt_cur = 0.1 * (i + 1);
            for (int q = 0; q < 3; ++q) pri[i].vel_prev[q] = 1.0 + i + 0.25 * q;
            pri[i].pose_before[0] = std::cos(0.15);  // a rotation about y by 0.3
            pri[i].pose_before[2] = std::sin(0.15);
            for (int q = 0; q < 3; ++q) pri[i].pose_before[4 + q] = 0.5 * i - q;
        }
        PackOptions po;
        po.pose_only = true;
        po.per_window_prior = true;
        po.window_priors = pri;
        po.prior = &pri[0];  // (ignored by a per-window batch)
        for (int i = 0; i < 3; ++i) {
            const WindowProblem pr = build_window_problem(W.get(), g_opts, po, i);
            CHECK(pr.rc == LIMO_OK);
            if (weight[i] > 0.0) {
                CHECK(pr.speed_w == weight[i] && pr.speed_dt == pri[i].dt_cur);
                for (int q = 0; q < 3; ++q) CHECK(pr.speed_vel[q] == pri[i].vel_prev[q] && pr.speed_tb[q] == pri[i].pose_before[4 + q]);
                const double c = std::cos(0.3), s = std::sin(0.3);
                const double Ry[9] = {c, 0, s, 0, 1, 0, -s, 0, c};
                for (int q = 0; q < 9; ++q) CHECK(std::fabs(pr.speed_Rb[q] - Ry[q]) < 1e-15);
            } else {
                CHECK(pr.speed_w == 0.0 && pr.speed_dt == 0.0);
                for (int q = 0; q < 9; ++q) CHECK(pr.speed_Rb[q] == 0.0);
            }
        }
        po.window_priors = nullptr;  // no array: no window has a prior
        CHECK(build_window_problem(W.get(), g_opts, po, 0).speed_w == 0.0);
        po.per_window_prior = false;  // the single call's way
        CHECK(build_window_problem(W.get(), g_opts, po, 2).speed_w == 0.7);
    }
    {   // what the rules refuse: code and message
        Win W(2, 3, 1);
        W.obs(0, 3, 0, -1.0f);
        WindowProblem pr = solve_problem(W);
        CHECK(pr.rc == LIMO_ERR_INVALID && std::string(pr.err) == "observation index out of range");
        Win E(0, 3, 1);
        pr = solve_problem(E);
        CHECK(pr.rc == LIMO_ERR_NOT_ENOUGH_KF && std::string(pr.err) == "window without active keyframes");
        PackOptions pp;
        pp.pose_only = true;
        Win T(2, 3, 1);
        pr = build_window_problem(T.get(), g_opts, pp, 0);
        CHECK(pr.rc == LIMO_ERR_INVALID && std::string(pr.err) == "pose-only window must hold exactly one keyframe");
    }
    {   // pack_windows refuses an evaluate-only batch with landmark shards (the evaluate chunks need every observation block on
        // the 64-grid of its view, and a sharded layout cuts blocks at shard runs); each option alone packs
        Win W(2, 12, 1);
        for (int l = 0; l < 12; ++l) W.obs(l % 2, l, 0, l % 3 ? -1.0f : 4.0f);
        const limo_ba_window w = W.get();
        PackedBatch P;
        std::string err;
        PackOptions po;
        po.evaluate_only = true;
        po.shards = 3;
        CHECK(pack_windows(1, &w, g_opts, po, P, err) == LIMO_ERR_INVALID);
        CHECK(err == "evaluate-only batch with landmark shards");
        po.shards = 1;
        CHECK(pack_windows(1, &w, g_opts, po, P, err) == LIMO_OK && P.n_echunk == 2);
        po.evaluate_only = false;
        po.shards = 3;
        CHECK(pack_windows(1, &w, g_opts, po, P, err) == LIMO_OK && P.n_shards == 3);
    }
}

int main() {
    std::memset(&g_opts, 0, sizeof(g_opts));
    g_opts.min_landmarks_for_trimming = 30;
    ground_plane();
    scale_regulariser();
    slots();
    landmark_states();
    views();
    trimming_prior_and_refusals();
    std::printf("%d checks, %d failed checks\n", g_checks, g_failed);
    return g_failed ? 1 : 0;
}
